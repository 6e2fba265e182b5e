"""CPU tests of the per-agent parameter entry points (sc_cbfqp_solve_batch_agents, sc_tracking_rollout_batch_agents) and of their
host side: symbols and version, argument validation before any device call, stack_robot_specs / agent_param_table, and the
controllers that refuse ``agent_spec``."""
import ctypes as C

import numpy as np
import pytest

import safe_control_amd as sca
from safe_control_amd import _lib, tracking as T
from safe_control_amd.position_control.cbf_qp import apply_cbf_overrides, default_cbf_param, make_params
from safe_control_amd.position_control.optimal_decay_cbf_qp import BatchedOptimalDecayCBFQP
from safe_control_amd.robots.spec import (AGENT_KEYS, agent_param_table, check_agent_spec, complete_robot_spec, stack_robot_specs,
                                          unstack_robot_specs)

from _agent_params_cases import SOLVE_MODELS, draw_agent_specs

# the two robots of the reference's examples/test_multi_robot.py:30-62
ROBOT_0 = {"model": "DynamicUnicycle2D", "w_max": 0.5, "a_max": 0.5, "sensor": "rgbd", "fov_angle": 45.0, "cam_range": 3.0,
           "radius": 0.25, "robot_id": 0}
ROBOT_1 = {"model": "DynamicUnicycle2D", "w_max": 1.0, "a_max": 1.5, "v_max": 2.0, "sensor": "rgbd", "fov_angle": 90.0,
           "cam_range": 5.0, "radius": 0.25, "robot_id": 1}
INVALID = _lib.SC_ERR_INVALID_ARGUMENT


def test_symbols_resolve_and_the_version_stays():
    lib = _lib.load()
    assert hasattr(lib, "sc_cbfqp_solve_batch_agents") and hasattr(lib, "sc_tracking_rollout_batch_agents")
    assert lib.sc_version() == _lib.ABI_VERSION == 9
    assert _lib.AGENT_PARAM_COLS == 10
    assert (_lib.AP_RADIUS, _lib.AP_ALPHA1, _lib.AP_ALPHA2, _lib.AP_U_MIN0, _lib.AP_U_MIN1, _lib.AP_U_MAX0, _lib.AP_U_MAX1,
            _lib.AP_V_MAX, _lib.AP_V_MIN, _lib.AP_REACHED) == tuple(range(10))


def test_header_and_binding_name_the_same_columns():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "safe_control_amd.h")).read()
    cols = dict(re.findall(r"#define SC_AP_([A-Z0-9_]+)\s+(\d+)", text))
    assert {k: int(v) for k, v in cols.items()} == {n[3:]: getattr(_lib, n) for n in dir(_lib) if n.startswith("AP_")}
    assert int(re.search(r"#define SC_AGENT_PARAM_COLS\s+(\d+)", text).group(1)) == _lib.AGENT_PARAM_COLS


def _qp_params(model_id=0):
    p = _lib.CbfQpParams()
    p.model_id, p.io_dtype, p.compute_dtype, p.dt, p.rear_ax_dist = model_id, 1, 1, 0.05, 0.2
    return p


def test_solve_argument_validation_without_a_device():
    lib = _lib.load()
    buf = np.zeros(256)
    ptr = buf.ctypes.data
    solve = lib.sc_cbfqp_solve_batch_agents
    msg = lambda: lib.sc_last_error().decode()
    p = _qp_params()
    assert solve(C.byref(p), 4, 8, ptr, ptr, ptr, None, None, ptr, ptr, None, None) == INVALID and "agent_params" in msg()
    assert solve(None, 4, 8, ptr, ptr, ptr, None, ptr, ptr, ptr, None, None) == INVALID and msg()
    for B in (0, -3):
        assert solve(C.byref(p), B, 8, ptr, ptr, ptr, None, ptr, ptr, ptr, None, None) == INVALID and "B <= 0" in msg()
    assert solve(C.byref(p), 4, _lib.CBFQP_MAX_OBS + 1, ptr, ptr, ptr, None, ptr, ptr, ptr, None, None) == INVALID
    assert "SC_CBFQP_MAX_OBS" in msg()
    assert solve(C.byref(p), 4, 0, ptr, ptr, ptr, None, ptr, ptr, ptr, None, None) == INVALID and msg()
    q = _qp_params(_lib.MODEL_IDS["Quad2D"])
    q.state_dim, q.mass = 6, 1.0
    assert solve(C.byref(q), 4, 8, ptr, ptr, ptr, None, ptr, ptr, ptr, None, None) == INVALID and "Quad2D" in msg()
    assert solve(C.byref(p), 4, 8, None, ptr, ptr, None, ptr, ptr, ptr, None, None) == INVALID and "NULL" in msg()


def _track_params(model_id=0, num_constraints=10):
    p = _lib.TrackingParams()
    p.qp = _qp_params(model_id)
    p.n_steps, p.max_waypoints, p.num_constraints = 5, 1, num_constraints
    p.reached_threshold, p.rotation_threshold, p.v_max, p.wheel_base = 0.3, 0.1, 1.0, 0.4
    return p


def test_rollout_argument_validation_without_a_device():
    lib = _lib.load()
    buf = np.zeros(256)
    ptr = buf.ctypes.data
    msg = lambda: lib.sc_last_error().decode()

    def roll(p, B, M, table, X=ptr):
        return lib.sc_tracking_rollout_batch_agents(C.byref(p) if p is not None else None, B, M, X, ptr, ptr, ptr, ptr, ptr, ptr, ptr,
                                                    ptr, ptr, None, None, table, None)
    p = _track_params()
    assert roll(p, 4, 2, None) == INVALID and "agent_params" in msg()
    assert roll(None, 4, 2, ptr) == INVALID and msg()
    for B in (0, -1):
        assert roll(p, B, 2, ptr) == INVALID and "B <= 0" in msg()
    for nc in (0, _lib.TRACKING_MAX_CONSTRAINTS + 1):
        assert roll(_track_params(num_constraints=nc), 4, 2, ptr) == INVALID and "num_constraints" in msg()
    assert roll(p, 4, -1, ptr) == INVALID and msg()
    assert roll(p, 4, 2, ptr, X=None) == INVALID and "NULL" in msg()
    q = _track_params(_lib.MODEL_IDS["Quad2D"])
    assert roll(q, 4, 2, ptr) != _lib.SC_OK and msg()             # the rollout has no Quad2D: refused as by its scalar sibling


def test_stack_round_trips_the_reference_example():
    shared, agent = stack_robot_specs([ROBOT_0, ROBOT_1])
    assert shared == {"model": "DynamicUnicycle2D", "sensor": "rgbd", "radius": 0.25}
    assert set(agent) == {"w_max", "a_max", "v_max", "fov_angle", "cam_range", "robot_id"}
    assert np.isnan(agent["v_max"][0]) and agent["v_max"][1] == 2.0          # robot 0 has no v_max: its default applies later
    assert unstack_robot_specs(shared, agent, 2) == [ROBOT_0, ROBOT_1]
    same, none = stack_robot_specs([ROBOT_0, dict(ROBOT_0)])
    assert same == ROBOT_0 and none == {}


def _scalar_columns(spec):
    """The table column a controller built from ``spec`` alone would send: make_params and _tracking_params of that one spec."""
    ctl = object.__new__(T.BatchedTrackingController)              # the host half only: no device tensor
    ctl._configure(dict(spec), 0.05, spec["model"] not in ("SingleIntegrator2D", "DoubleIntegrator2D"), False, "f64", "cuda:0")
    ctl.cbf_param = apply_cbf_overrides(default_cbf_param(spec["model"]), ctl.robot_spec)
    ctl.waypoints, ctl.steps_done = np.zeros((1, 1, 2)), 0
    t = ctl._tracking_params(1)
    rs = complete_robot_spec(dict(spec))
    q = make_params(rs, apply_cbf_overrides(default_cbf_param(rs["model"]), rs), 0.05, rs["radius"], _lib.DTYPE_F64, _lib.DTYPE_F64)
    for a, b in ((q.robot_radius, t.qp.robot_radius), (q.alpha1, t.qp.alpha1), (q.u_max[1], t.qp.u_max[1])):
        assert a == b
    return [q.robot_radius, q.alpha1, q.alpha2, q.u_min[0], q.u_min[1], q.u_max[0], q.u_max[1], t.v_max, t.v_min, t.reached_threshold]


@pytest.mark.parametrize("name", SOLVE_MODELS)
def test_table_columns_equal_the_single_spec_structs(name):
    specs = draw_agent_specs(name, 9, np.random.default_rng(5))
    specs[3] = {"model": name}                                       # every default
    specs[4] = {"model": name, "radius": 0.31}
    shared, agent = stack_robot_specs(specs)
    table = agent_param_table(shared, agent, len(specs))
    assert table.shape == (_lib.AGENT_PARAM_COLS, len(specs)) and table.dtype == np.float64
    for i, s in enumerate(specs):
        assert table[:, i].tolist() == _scalar_columns(s), (name, i)


def test_reference_example_table():
    shared, agent = stack_robot_specs([ROBOT_0, ROBOT_1])
    table = agent_param_table(shared, agent, 2)
    assert table[:, 0].tolist() == _scalar_columns(ROBOT_0) and table[:, 1].tolist() == _scalar_columns(ROBOT_1)
    assert table[_lib.AP_V_MAX].tolist() == [1.0, 2.0] and table[_lib.AP_U_MAX0].tolist() == [0.5, 1.5]


def test_stack_refuses_keys_that_may_not_vary():
    for key, a, b in (("model", "DynamicUnicycle2D", "Unicycle2D"), ("num_constraints", 8, 10), ("rear_ax_dist", 0.2, 0.3)):
        with pytest.raises(ValueError, match=key):
            stack_robot_specs([dict(ROBOT_0, **{key: a}), dict(ROBOT_0, **{key: b})])
    with pytest.raises(ValueError, match="num_constraints"):          # present in one spec only
        stack_robot_specs([dict(ROBOT_0, num_constraints=8), ROBOT_0])
    with pytest.raises(ValueError, match="mass"):
        check_agent_spec({"mass": [1.0, 2.0]}, 2)
    assert "radius" in AGENT_KEYS and "model" not in AGENT_KEYS


def test_table_refuses_bad_values():
    shared, agent = stack_robot_specs([ROBOT_0, ROBOT_1])
    for key, bad in (("a_max", -1.0), ("w_max", float("inf")), ("v_max", -2.0)):
        a = {k: v.copy() for k, v in agent.items()}
        a.setdefault(key, np.array([1.0, 1.0]))
        a[key][1] = bad
        with pytest.raises(ValueError):
            agent_param_table(shared, a, 2)
    with pytest.raises(ValueError):
        stack_robot_specs([dict(ROBOT_0, radius=float("nan")), ROBOT_1])


def test_wrong_length_raises():
    shared, agent = stack_robot_specs([ROBOT_0, ROBOT_1])
    with pytest.raises(ValueError, match="2 entries for a batch of 3"):
        agent_param_table(shared, agent, 3)
    with pytest.raises(ValueError, match="batch of 3"):                # before the first device tensor
        sca.BatchedTrackingController(np.zeros((3, 3)), dict(shared), agent_spec=agent)
    with pytest.raises(ValueError, match="same number of agents"):
        sca.BatchedCBFQP(dict(shared), io_dtype="f64", agent_spec={"a_max": [0.5, 1.5], "w_max": [0.5, 1.0, 1.0]})


def test_controllers_that_do_not_serve_agent_spec_say_so():
    shared, agent = stack_robot_specs([ROBOT_0, ROBOT_1])
    X0 = np.zeros((2, 3))
    served = "served by the 'cbf_qp' solve"
    for pos in ("optimal_decay_cbf_qp", "mpc_cbf", "optimal_decay_mpc_cbf"):
        with pytest.raises(ValueError, match=served):
            sca.BatchedTrackingController(X0, dict(shared), controller_type={"pos": pos}, agent_spec=agent)
    for model in ("Quad2D", "Quad3D", "VTOL2D"):
        with pytest.raises(ValueError, match=served):
            sca.BatchedTrackingController(X0, {"model": model}, agent_spec=agent)
    with pytest.raises(ValueError, match=served):
        T.BatchedQuadTrackingController(X0, {"model": "Quad2D"}, controller_type={"pos": "cbf_qp"}, agent_spec=agent)
    for cls in (T.BatchedSensingTrackingController, T.BatchedSensingMPCTrackingController, T.BatchedFleetTrackingController):
        with pytest.raises(ValueError, match=served):
            cls(X0, dict(shared), agent_spec=agent)
    with pytest.raises(ValueError, match=served):
        BatchedOptimalDecayCBFQP(dict(shared), agent_spec=agent)
    with pytest.raises(ValueError, match="Quad2D"):
        sca.BatchedCBFQP({"model": "Quad2D"}, io_dtype="f64", agent_spec={"radius": [0.2, 0.3]})
    with pytest.raises(ValueError, match="f64"):
        sca.BatchedCBFQP(dict(shared), io_dtype="f32", compute_dtype="f32", agent_spec=agent)
