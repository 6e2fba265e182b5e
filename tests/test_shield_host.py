"""CPU: the host logic the Gatekeeper / MPS shields share (safe_control_amd/shielding/_shield_host.py) under the classes of both
scenarios.  The library loads without a GPU, and constructors, ``params()`` and the input checks run before any HIP call: the bytes
of ``params`` against a struct filled here field by field from the documented constructor arguments; ``fields()`` as a partition of
the state buffer; every input check with the class's own text (on stand-in tensors that say they are device tensors); the drop-ins'
transposition rule, their getters before the first call, their refusals and the MPS constructors."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from safe_control_amd import _lib, shielding  # noqa: E402
from safe_control_amd.shielding import _shield_host, drift, gatekeeper, mps  # noqa: E402

ALGOS = {"gatekeeper": _lib.SHIELD_GATEKEEPER, "mps": _lib.SHIELD_MPS}
IO = {"f32": (_lib.DTYPE_F32, torch.float32), "f64": (_lib.DTYPE_F64, torch.float64)}
ENV = dict(hallway_length=61.0, half_width=2.5, pocket_x_min=24.0, pocket_x_max=33.0, pocket_y_min=2.5, pocket_y_max=6.25, goal_x_min=57.0,
           goal_x_max=61.0, bullet_speed=3.5, bullet_length=2.75, bullet_width=4.5, bullet_start_x=-9.0)
TIMES = dict(dt=0.08, backup_horizon=1.3, nominal_horizon=0.9, event_offset=0.07, safety_margin=0.3, horizon_discount=0.25)
COUNTS = dict(n_backup=16, n_nominal=11, discount_steps=3)            # int(1.3 / 0.08), int(0.9 / 0.08), int(0.25 / 0.08)


def evade(algo="gatekeeper", io="f64", **kw):
    return shielding.BatchedShield(algo, {"radius": 0.45, "a_max": 1.75, "v_max": 1.25}, ENV, predict_bullet=False, io_dtype=io, kp=1.5, kd=2.5,
                                   **dict(TIMES, **kw))


SPEC = dict(drift.default_robot_spec(), a=1.3, b=1.5, m=2400.0, Iz=5100.0, Cc_f=81000.0, Cc_r=99000.0, mu=0.9, r_w=0.34, gamma=0.94, delta_max=0.36,
            delta_dot_max=0.45, tau_max=3900.0, tau_dot_max=7900.0, v_max=21.0, v_min=0.5, r_max=1.9, beta_max=0.8, radius=1.25, v_ref=9.0)
TRACK = dict(track_type="straight", track_length=310.0, track_width=18.0, num_lanes=6)
PUDDLES = [(50.0, -2.0, 10.0, 4.0), (120.0, 3.0, 8.0, 2.0)]


def drift_car(algo="gatekeeper", io="f64", backup="lane_change", **kw):
    return drift.BatchedDriftShield(algo, backup, SPEC, TRACK, io_dtype=io, ego_lane=2, backup_lane=4, puddles=PUDDLES, **dict(TIMES, **kw))


def test_algo_id_and_counts():
    assert not hasattr(gatekeeper, "_algo_id") and not hasattr(drift, "_algo_id")          # one copy
    for name, want in ALGOS.items():
        assert _shield_host.algo_id(name) == want
    for make in (evade, drift_car):
        with pytest.raises(ValueError, match=re.escape("algo must be one of ['gatekeeper', 'mps']")):
            make("backupcbf")
        sh = make()
        assert {k: getattr(sh, k) for k in COUNTS} == COUNTS and sh.max_nominal == 11
        assert make(max_nominal=7).max_nominal == 7
        sh = make(nominal_horizon=0.0)
        assert (sh.n_nominal, sh.max_nominal) == (0, 1)
        for io, (code, dt_) in IO.items():
            assert (make(io=io).io_dtype, make(io=io).torch_dtype) == (code, dt_)
        assert make(io="float32").io_dtype == _lib.DTYPE_F32
    assert shielding.BatchedShield(dt=0.1).discount_steps == 5 and drift.BatchedDriftShield(dt=0.05).discount_steps == 5     # 5 dt


@pytest.mark.parametrize("io", list(IO))
@pytest.mark.parametrize("algo", list(ALGOS))
def test_evade_params_field_by_field(algo, io):
    sh = evade(algo, io)
    for kw, n_nominal, shared in (({}, 11, 0), (dict(n_nominal=4, bullet_shared=True), 4, 1), (dict(n_nominal=0, bullet_shared=False), 0, 0)):
        want = _lib.ShieldParams()
        want.algo, want.n_nominal, want.max_nominal, want.n_backup, want.discount_steps = ALGOS[algo], n_nominal, 11, 16, 3
        want.predict_bullet, want.event_offset = 0, 0.07
        b = want.base
        b.io_dtype, b.n_steps, b.bullet_shared = IO[io][0], 16, shared
        b.dt, b.robot_radius, b.a_max, b.v_max, b.safety_margin, b.backup_kp, b.backup_kd = 0.08, 0.45, 1.75, 1.25, 0.3, 1.5, 2.5
        for k, v in ENV.items():
            setattr(b, k, v)
        assert bytes(sh.params(**kw)) == bytes(want), kw
    sh.predict_bullet = True                                                  # the drop-in sets it per call
    assert sh.params().predict_bullet == 1
    assert sh.params(5).n_nominal == 5                                        # positional, as the drop-in passes it


def _controller(kind, **num):
    c = _lib.DriftController()
    c.kind = kind
    for k, v in num.items():
        assert k in _lib.DRIFT_CTRL_KEYS
        setattr(c, k, v)
    return c


def _lane_change(target_y):                                                  # LaneChangeController's numbers (backup_controller.py:102-124)
    return _controller(_lib.DRIFT_LANE_CHANGE, target_y=target_y, kp_y=0.25, kd_y=0.3, kp_theta=1.2, kd_theta=1.0, kp_delta=2.5, kp_v=500.0,
                       kp_tau_dot=2.0, v_target=9.0, theta_des_max=np.radians(20), delta_max=0.36, delta_dot_max=0.45, tau_max=3900.0,
                       tau_dot_max=7900.0)


@pytest.mark.parametrize("io", list(IO))
@pytest.mark.parametrize("backup", ["lane_change", "stop"])
@pytest.mark.parametrize("algo", list(ALGOS))
def test_drift_params_field_by_field(algo, backup, io):
    sh = drift_car(algo, io, backup)
    lane = lambda i: 9.0 - (i + 0.5) * 3.0                                    # width 18, six lanes
    for kw, got in (({}, (11, 0, 0, 0)), (dict(n_nominal=4, n_static=2, n_moving=3, obs_shared=True), (4, 2, 3, 1))):
        want = _lib.DriftShieldParams()
        want.algo, want.io_dtype, want.track_type = ALGOS[algo], IO[io][0], _lib.DRIFT_TRACK_STRAIGHT
        want.n_nominal, want.n_static, want.n_moving, want.obs_shared = got
        want.max_nominal, want.n_backup, want.discount_steps, want.n_puddles = 11, 16, 3, 2
        want.dt, want.event_offset, want.safety_margin, want.robot_radius = 0.08, 0.07, 0.3, 1.25
        for k in _lib.DRIFT_VEHICLE_KEYS:
            setattr(want, k, SPEC[k])
        want.track_length, want.track_width, want.mu_default = 310.0, 18.0, 0.9
        for i, row in enumerate(PUDDLES):
            for j in range(4):
                want.puddles[i][j] = row[j]
        want.keeper = _lane_change(lane(2))
        want.backup = _lane_change(lane(4)) if backup == "lane_change" else _controller(
            _lib.DRIFT_STOP, kp_v=1000.0, kd_theta=1.0, kp_delta=3.0, stop_velocity=0.05, min_braking_torque=-500.0, holding_torque=-100.0,
            delta_max=0.36, delta_dot_max=0.45, tau_max=3900.0, tau_dot_max=7900.0)
        assert bytes(sh.params(**kw)) == bytes(want), kw
    assert bytes(sh.params(4, 2, 3, True)) == bytes(sh.params(n_nominal=4, n_static=2, n_moving=3, obs_shared=True))      # the drop-in's order


@pytest.mark.parametrize("C_", [1, 7])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("algo", list(ALGOS))
@pytest.mark.parametrize("make,nx,extra", [(evade, 4, ()), (drift_car, 8, ("commit_friction",))], ids=["evade", "drift"])
def test_fields_partition_the_state_buffer(make, nx, extra, algo, B, C_):
    sh = make(algo, max_nominal=C_, nominal_horizon=0.0)                       # (n_nominal <= max_nominal)
    nbytes = sh.state_bytes(B)
    assert nbytes == B * (C_ * 16 + nx * 8 + 8 * len(extra) + 8 + 16)         # include/safe_control_amd.h
    state = torch.zeros(nbytes, dtype=torch.uint8)
    f = sh.fields(state, B)
    doc = {"cu": (torch.float64, (B, C_, 2)), "cursor": (torch.float64, (B, nx)), "net": (torch.float64, (B,)),
           **{k: (torch.float64, (B,)) for k in extra}, **{k: (torch.int32, (B,)) for k in ("s", "idx", "clen", "init")}}
    assert set(f) == set(doc) and ("commit_friction" in f) == (make is drift_car)
    base, covered, order = state.data_ptr(), np.zeros(nbytes, dtype=np.int64), []
    for k, (dt_, shape) in doc.items():
        assert f[k].dtype == dt_ and tuple(f[k].shape) == shape and f[k].is_contiguous(), k
        lo = f[k].data_ptr() - base
        covered[lo:lo + f[k].numel() * f[k].element_size()] += 1
        order.append((lo, k))
    assert (covered == 1).all()                                               # disjoint, and together the whole buffer
    assert [k for _, k in sorted(order)] == ["cu", "cursor", *extra, "net", "s", "idx", "clen", "init"]
    f["idx"][B - 1] = 5                                                       # views, not copies
    assert state.view(torch.int32)[-2 * B - 1] == 5


class Dev:
    """Stands in for a device tensor where the checks read nothing but these."""

    def __init__(self, shape, dtype=torch.float64, cuda=True, contiguous=True):
        self.shape, self.dtype, self.is_cuda, self._contiguous = tuple(shape), dtype, cuda, contiguous

    def is_contiguous(self):
        return self._contiguous

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape))


STATE_TEXT = "state must be a contiguous CUDA buffer of state_bytes(B) bytes (new_state(B))"


def _tensor_cases(good, k, dt_):
    other = torch.float32 if dt_ == torch.float64 else torch.float64
    return (torch.zeros(good[k], dtype=dt_), Dev(good[k], dtype=other), Dev(good[k], dtype=dt_, contiguous=False))      # host, dtype, strided


def _state_cases(sh, B):
    n = sh.state_bytes(B)
    return (torch.zeros(n, dtype=torch.uint8), Dev((n + 1,), torch.uint8), Dev((n,), torch.uint8, contiguous=False), Dev((sh.state_bytes(B + 1),), torch.uint8))


@pytest.mark.parametrize("io", list(IO))
@pytest.mark.parametrize("algo", list(ALGOS))
def test_evade_input_checks(algo, io):
    sh, dt_, B, M = evade(algo, io), IO[io][1], 3, 5
    good = {"X": (B, 4), "bullet_x": (B,), "nominal_x": (B, M + 1, 4), "nominal_u": (B, M, 2)}
    state = Dev((sh.state_bytes(B),), torch.uint8)
    call = lambda **over: sh.step(*[over.get(k, Dev(good[k], dt_)) for k in ("X", "bullet_x")], over.get("state", state),
                                  *[over.get(k, Dev(good[k], dt_)) for k in ("nominal_x", "nominal_u")])
    assert sh._check(Dev(good["X"], dt_), Dev(good["bullet_x"], dt_), state) == B
    assert sh._check(Dev(good["X"], dt_), Dev((1,), dt_), state, ("nominal_x", None)) == B
    for k in good:
        for bad in _tensor_cases(good, k, dt_):
            with pytest.raises(ValueError, match=re.escape(f"{k} must be a contiguous CUDA tensor of dtype {dt_}")):
                call(**{k: bad})
    for over in (dict(X=Dev((B, 5), dt_)), dict(X=Dev((B, 4, 1), dt_)), dict(bullet_x=Dev((2,), dt_)), dict(bullet_x=Dev((B + 1,), dt_))):
        with pytest.raises(ValueError, match=re.escape("expected X[B,4], bullet_x[B] or [1]")):
            call(**over)
    for bad in _state_cases(sh, B):
        with pytest.raises(ValueError, match=re.escape(STATE_TEXT)):
            call(state=bad)
    text = re.escape("expected nominal_x[B, M+1, 4] and nominal_u[B, M, 2]")
    for over in (dict(nominal_x=Dev((B, M + 1, 8), dt_)), dict(nominal_x=Dev((B + 1, M + 1, 4), dt_)), dict(nominal_u=Dev((B, M - 1, 2), dt_)),
                 dict(nominal_u=Dev((B, M, 3), dt_)), dict(nominal_u=None)):
        with pytest.raises(ValueError, match=text):
            call(**over)
    ints = Dev((B,), torch.int32)
    with pytest.raises(ValueError, match=re.escape("rollout needs one bullet position per agent (bullet_x[B])")):
        sh.rollout(Dev(good["X"], dt_), Dev((1,), dt_), state, ints, ints, 1)
    with pytest.raises(ValueError, match=re.escape(STATE_TEXT)):
        sh.rollout(Dev(good["X"], dt_), Dev((B,), dt_), Dev((7,), torch.uint8), ints, ints, 1)
    q = evade(algo, io, max_nominal=_lib.SHIELD_MAX_NOMINAL + 1)
    with pytest.raises(ValueError, match="invalid shield parameters"):
        q.state_bytes(1)
    assert q.state_bytes(0) == 0


@pytest.mark.parametrize("io", list(IO))
@pytest.mark.parametrize("algo", list(ALGOS))
def test_drift_input_checks(algo, io):
    sh, dt_, B, M = drift_car(algo, io), IO[io][1], 3, 5
    good = {"X": (B, 8), "friction": (B,), "nominal_x": (B, M + 1, 8), "nominal_u": (B, M, 2), "static_obs": (B, 2, 3), "moving_obs": (B, 2, 7)}
    state = Dev((sh.state_bytes(B),), torch.uint8)
    order = ("X", "friction", "state", "nominal_x", "nominal_u", "static_obs", "moving_obs")
    call = lambda **over: sh.step(*[over.get(k, state if k == "state" else Dev(good[k], dt_)) for k in order])
    T = lambda *shape: Dev(shape, dt_)
    assert sh._check(T(B, 8), T(B), state, T(B, 2, 3), T(B, 1, 7)) == (B, 2, 1, False)
    assert sh._check(T(B, 8), T(B), state, T(2, 3), T(4, 7)) == (B, 2, 4, True)
    assert sh._check(T(B, 8), T(B), state, None, T(B, 0, 7)) == (B, 0, 0, False)
    for k in good:
        for bad in _tensor_cases(good, k, dt_):
            with pytest.raises(ValueError, match=re.escape(f"{k} must be a contiguous CUDA tensor of dtype {dt_}")):
                call(**{k: bad})
    for over in (dict(X=T(B, 4)), dict(friction=T(1)), dict(friction=T(B, 1))):
        with pytest.raises(ValueError, match=re.escape("expected X[B,8], friction[B]")):
            call(**over)
    for bad in _state_cases(sh, B):
        with pytest.raises(ValueError, match=re.escape(STATE_TEXT)):
            call(state=bad)
    for k, w in (("static_obs", 3), ("moving_obs", 7)):
        for shape in ((B, 2, w + 1), (B + 1, 2, w), (w,), (1, B, 2, w)):
            with pytest.raises(ValueError, match=re.escape(f"expected {k}[B, n, {w}] or [n, {w}]")):
                call(**{k: T(*shape)})
        with pytest.raises(NotImplementedError, match=f"more than {_lib.DRIFT_MAX_OBS} obstacles in {k}"):
            call(**{k: T(B, _lib.DRIFT_MAX_OBS + 1, w)})
    with pytest.raises(ValueError, match="static_obs and moving_obs must both be per car or both shared"):
        call(static_obs=T(2, 3))
    text = re.escape("expected nominal_x[B, M+1, 8] and nominal_u[B, M, 2]")
    for over in (dict(nominal_x=T(B, M + 1, 4)), dict(nominal_x=T(B + 1, M + 1, 8)), dict(nominal_u=T(B, M + 1, 2)), dict(nominal_u=None)):
        with pytest.raises(ValueError, match=text):
            call(**over)
    ints = Dev((B,), torch.int32)
    with pytest.raises(ValueError, match=re.escape("rollout moves the obstacles: it needs one table per car ([B, n, .])")):
        sh.rollout(T(B, 8), T(B), T(2, 7), state, ints, ints, 1, static_obs=T(1, 3))
    q = drift_car(algo, io, max_nominal=_lib.DRIFT_MAX_NOMINAL + 1)
    with pytest.raises(ValueError, match="invalid drift shield parameters"):
        q.state_bytes(1)


# ---- the drop-ins ---------------------------------------------------------------------------------------------------------------
class _Env:
    bullet_x, bullet_active, track_type, track_length, track_width, num_lanes, obstacles = -10.0, True, "straight", 300.0, 20.0, 5, ()


class _EvadeBackup:
    safe_center, safe_bounds, Kp, Kd, a_max, goal_bounds = np.array([30.0, 4.0]), {}, 2.0, 2.0, 2.0, {}


class StoppingController:
    Kp_v, Kd_theta, Kp_delta, stop_velocity_threshold, min_braking_torque, holding_torque = 1000.0, 1.0, 3.0, 0.05, -500.0, -100.0
    delta_max, delta_dot_max, tau_max, tau_dot_max = 0.35, 0.44, 4000.0, 8000.0


DROP_INS = [(shielding.Gatekeeper, 4, {"model": "DoubleIntegrator2D", "a_max": 2.0}, _EvadeBackup, "the native shields"),
            (shielding.MPS, 4, {"model": "DoubleIntegrator2D", "a_max": 2.0}, _EvadeBackup, "the native shields"),
            (drift.Gatekeeper, 8, {"model": "DriftingCar"}, StoppingController, "the native drift shields"),
            (drift.MPS, 8, {"model": "DriftingCar"}, StoppingController, "the native drift shields")]
DROP_IDS = ["evade-gatekeeper", "evade-mps", "drift-gatekeeper", "drift-mps"]


def test_public_names_and_constructors():
    assert shielding.Gatekeeper is gatekeeper.Gatekeeper and shielding.MPS is mps.MPS and shielding.BatchedShield is gatekeeper.BatchedShield
    assert issubclass(mps.MPS, gatekeeper.Gatekeeper) and issubclass(drift.MPS, drift.Gatekeeper) and not issubclass(drift.MPS, gatekeeper.Gatekeeper)
    gk = "(self, robot, robot_spec, dt=0.05, backup_horizon=2.0, event_offset=0.5, ax=None, nominal_horizon=None, horizon_discount=None, safety_margin=1.0, device=0)"
    ms = "(self, robot, robot_spec, dt=0.05, backup_horizon=2.0, event_offset=0.5, ax=None, safety_margin=1.0, device=0)"
    for cls, want in ((gatekeeper.Gatekeeper, gk), (drift.Gatekeeper, gk), (mps.MPS, ms), (drift.MPS, ms)):
        assert str(inspect.signature(cls.__init__)) == want, cls
    for name in ("default_robot_spec", "default_track", "lane_center", "lane_change_controller", "stopping_controller", "controller_from_object",
                 "DRIFT_MODELS", "BatchedDriftShield"):
        assert hasattr(drift, name), name


@pytest.mark.parametrize("cls,n,spec,backup,served", DROP_INS, ids=DROP_IDS)
def test_drop_in_constructor_fields_and_getters_before_the_first_call(cls, n, spec, backup, served):
    robot = object()
    is_mps = cls._algo == "mps"
    sh = cls(robot, spec, 0.1, 1.5, 0.2, None, safety_margin=0.4, device=1) if is_mps else cls(robot, spec, 0.1, 1.5, 0.2, None, 2.5, 0.3, 0.4, 1)
    assert sh.robot is robot and sh.robot_spec is spec and (sh.dt, sh.backup_horizon, sh.event_offset, sh.safety_margin, sh._device) == (0.1, 1.5, 0.2, 0.4, 1)
    assert (sh.nominal_horizon, sh.horizon_discount) == ((1.5, 0.5) if is_mps else (2.5, 0.3))       # MPS: the defaults (backup_horizon, 5 dt)
    assert (sh.n_states, sh.n_controls, sh._algo) == (n, 2, "mps" if is_mps else "gatekeeper")
    for k in ("nominal_controller", "backup_controller", "backup_target", "env", "moving_obstacles", "nominal_x_traj", "nominal_u_traj",
              "committed_x_traj", "committed_u_traj"):
        assert getattr(sh, k) is None, k
    assert (sh.next_event_time, sh.current_time_idx, sh.committed_horizon, sh.actual_nominal_steps) == (0.0, 15, 0.0, 0)
    assert sh.get_status() == {"current_time_idx": 15, "committed_horizon": 0.0, "next_event_time": 0.0, "using_backup": True, "committed_length": 0}
    assert sh.get_committed_trajectory() == (None, None) and sh.get_committed_horizon() == 0.0 and sh.is_using_backup() is True
    assert cls(robot, spec).horizon_discount == 0.25 and cls(robot, spec).current_time_idx == 40
    sh.set_moving_obstacles(len)
    assert sh.moving_obstacles is len


@pytest.mark.parametrize("cls,n,spec,backup,served", DROP_INS, ids=DROP_IDS)
def test_drop_in_transposition_rule(cls, n, spec, backup, served):
    sh, M = cls(None, spec), 9
    xs, us = np.arange(float(n * (M + 1))).reshape(M + 1, n), np.arange(2.0 * M).reshape(M, 2)
    for x_in, u_in in ((xs, us), (xs.T, us.T), (xs.T.tolist(), us)):          # [M+1, n], [n, M+1]: rows < columns is transposed
        sh.set_nominal_trajectory(x_in, u_in)
        assert np.array_equal(sh.nominal_x_traj, xs) and np.array_equal(sh.nominal_u_traj, us)
    assert sh.nominal_x_traj is not xs                                        # a copy
    sh.set_nominal_trajectory(None, us[:3])                                   # None leaves a trajectory as it is
    assert np.array_equal(sh.nominal_x_traj, xs) and np.array_equal(sh.nominal_u_traj, us[:3])
    sh.set_nominal_trajectory(xs[:n], us[:2])                                 # square: as it came
    assert np.array_equal(sh.nominal_x_traj, xs[:n]) and np.array_equal(sh.nominal_u_traj, us[:2])
    sh.set_nominal_trajectory(xs[:2], None)                                   # the rule is the reference's: two states of n > 2 columns are transposed
    assert sh.nominal_x_traj.shape == (n, 2)


@pytest.mark.parametrize("cls,n,spec,backup,served", DROP_INS, ids=DROP_IDS)
def test_drop_in_refusals_before_any_launch(cls, n, spec, backup, served):
    sh, M = cls(None, spec), 6
    x = np.zeros(n)
    with pytest.raises(NotImplementedError, match=re.escape(f"{served} need the external nominal trajectory (set_nominal_trajectory)")):
        sh.solve_control_problem(x)
    sh.set_nominal_trajectory(np.zeros((M + 1, n)), None)
    with pytest.raises(NotImplementedError, match="need the external nominal trajectory"):
        sh.solve_control_problem(x)
    sh.set_nominal_trajectory(None, np.zeros((M - 1, 2)))
    with pytest.raises(ValueError, match="nominal_u_traj is shorter than nominal_x_traj - 1"):
        sh.solve_control_problem(x)
    sh.set_nominal_trajectory(None, np.zeros((M, 2)))
    with pytest.raises(RuntimeError, match=re.escape("set_environment() and set_backup_controller() first")):
        sh.solve_control_problem(x)
    sh.set_environment(_Env())
    with pytest.raises(RuntimeError, match="first"):
        sh.solve_control_problem(x, friction=0.8)
    sh.set_backup_controller(backup(), target=-4.0)
    assert sh.backup_target == -4.0 and sh._batched is None and sh._state is None
    sh.set_nominal_controller(lambda s: np.zeros((2, 1)))
    with pytest.raises(NotImplementedError, match=re.escape("forward-propagation mode (set_nominal_controller) is not served: pass set_nominal_trajectory")):
        sh.solve_control_problem(x)
    with pytest.raises(NotImplementedError):
        sh.set_backup_controller(object())


def test_evade_drop_in_refusals():
    for cls in (shielding.Gatekeeper, shielding.MPS):
        for spec in ({"model": "DynamicBicycle2D"}, {}, {"model": "Quad3D"}):     # the reference's default model is not served either
            with pytest.raises(NotImplementedError, match=re.escape("the native shields serve DoubleIntegrator2D (the evade scenario)")):
                cls(None, spec)
        sh = cls(None, {"model": "double_integrator", "a_max": 2.0})
        b = _EvadeBackup()
        b.goal_bounds = None
        with pytest.raises(NotImplementedError, match="goal_bounds=None"):
            sh.set_backup_controller(b)
        b = _EvadeBackup()
        b.a_max = 2.5
        with pytest.raises(NotImplementedError, match=re.escape("backup controller a_max differs from robot_spec['a_max']")):
            sh.set_backup_controller(b)
        assert sh.backup_controller is None
        env = _Env()
        env.bullet_active = False
        sh.set_environment(env)
        sh.set_backup_controller(_EvadeBackup())
        sh.set_nominal_trajectory(np.zeros((4, 4)), np.zeros((3, 2)))
        with pytest.raises(NotImplementedError, match="the native shields expect the evade scenario's active bullet"):
            sh.solve_control_problem(np.zeros(4))
    with pytest.raises(NotImplementedError, match="the native shields serve DoubleIntegrator2D"):
        shielding.BatchedShield("gatekeeper", robot_spec={"model": "Quad3D"})


def test_evade_predictor_is_the_examples():
    sh = shielding.Gatekeeper(None, {"model": "DoubleIntegrator2D"})
    env = _Env()
    env.bullet_length, env.bullet_width, env.bullet_speed = 3.0, 4.0, 3.0
    sh.set_environment(env)
    assert sh._predictor() is False                                           # no predictor: the bullet now only
    box = dict(x=-10.0 + 0.5, y=0.0, length=4.0, width=4.0, vx=3.0)
    sh.set_moving_obstacles(lambda t=0.0: dict(box))
    assert sh._predictor() is True
    sh.set_moving_obstacles(dict(box, length=3.0))
    with pytest.raises(NotImplementedError, match="the native shields serve the evade example's bullet predictor"):
        sh._predictor()


def test_drift_drop_in_refusals_and_tables():
    for cls in (drift.Gatekeeper, drift.MPS):
        with pytest.raises(NotImplementedError, match="the native drift shields serve the DriftingCar on DynamicBicycle2D"):
            cls(None, {"model": "DoubleIntegrator2D"})
        sh = cls(None, {})                                                    # the reference's default model
        for tt in ("oval", "l_shape"):
            env = _Env()
            env.track_type = tt
            with pytest.raises(NotImplementedError, match="the native drift shields serve the straight track only"):
                sh.set_environment(env)
        env = _Env()
        env.obstacles = [{"x": 1.0 * i, "y": 0.0, "spec": {}} for i in range(_lib.DRIFT_MAX_OBS + 1)]
        with pytest.raises(NotImplementedError, match=f"more than {_lib.DRIFT_MAX_OBS} static obstacles"):
            sh.set_environment(env)
        assert sh.env is None
        env.obstacles = [{"x": 40.0, "y": -4.0, "spec": {"radius": 2.0}}, {"x": 80.0, "y": 4.0, "spec": {}}]
        sh.set_environment(env)
        assert np.array_equal(sh._static_table(), [[40.0, -4.0, 2.0], [80.0, 4.0, 2.5]]) and sh._moving_table().shape == (0, 7)
        car = lambda t=0.0: [dict(x=10.0 + 3.0 * t, y=1.0 - 0.5 * t, vx=3.0, vy=-0.5, length=4.0, width=2.0, radius=1.5), None]
        sh.set_moving_obstacles(car)
        assert np.array_equal(sh._moving_table(), [[10.0, 1.0, 3.0, -0.5, 4.0, 2.0, 1.5]])
        sh.set_moving_obstacles(lambda t=0.0: [dict(x=10.0 + t * t, y=0.0, vx=3.0, vy=0.0, length=4.0, width=2.0)])
        with pytest.raises(NotImplementedError, match="not constant-velocity"):
            sh._moving_table()
        sh.set_moving_obstacles(lambda t=0.0: [dict(car()[0])] * (_lib.DRIFT_MAX_OBS + 1))
        with pytest.raises(NotImplementedError, match=f"more than {_lib.DRIFT_MAX_OBS} moving obstacles"):
            sh._moving_table()
        with pytest.raises(ValueError, match="the lane-change backup needs its target lane centre"):
            sh.set_backup_controller(type("LaneChangeController", (), {})())
        sh.set_backup_controller(StoppingController())
        assert sh._ctrl["kind"] == "stop" and sh._ctrl["kp_v"] == 1000.0
    for kw in (dict(robot_spec={"model": "DoubleIntegrator2D"}), dict(track={"track_type": "oval"}), dict(backup="evade"),
               dict(puddles=[(0.0, 0.0, 1.0, 1.0)] * (_lib.DRIFT_MAX_PUDDLES + 1))):
        with pytest.raises(NotImplementedError):
            drift.BatchedDriftShield("gatekeeper", **kw)


def test_the_drop_ins_reach_the_library_through_the_batched_class_only():
    for f in ("gatekeeper", "mps", "drift"):
        src = open(os.path.join(ROOT, "safe_control_amd", "shielding", f + ".py")).read()
        assert "_lib.sc_" not in src and "data_ptr" not in src and "import ctypes" not in src, f
    assert _shield_host.BatchedShieldBase._step is shielding.BatchedShield._step is drift.BatchedDriftShield._step
