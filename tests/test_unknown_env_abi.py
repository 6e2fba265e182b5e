"""CPU: the sensing rollout's entry point (sc_tracking_sense_rollout_batch) exists with its argument types, sc_sense_params
compiles as C99 with the size and offsets of the ctypes mirror, bad arguments are refused before any HIP call, the ABI version
did not move (the entry point is an addition), and BatchedSensingTrackingController checks its arguments before it creates a
device tensor -- while the base class still refuses a rotating integrator."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import safe_control_amd as sca
from safe_control_amd import _lib
from safe_control_amd.position_control.cbf_qp import apply_cbf_overrides, default_cbf_param, make_params
from safe_control_amd.robots.spec import complete_robot_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, 1, 2


def tracking_params(model="DoubleIntegrator2D", **over):
    rs = complete_robot_spec({"model": model, "radius": 0.25})
    p = _lib.TrackingParams()
    p.qp = make_params(rs, apply_cbf_overrides(default_cbf_param(model), rs), 0.05, rs["radius"], _lib.DTYPE_F64, _lib.DTYPE_F64)
    p.n_steps, p.max_waypoints, p.enable_rotation, p.num_constraints = 1, 4, 1, 10
    p.reached_threshold, p.rotation_threshold, p.v_max = 0.3, 0.1, 1.0
    p.k_omega, p.k_a, p.k_v = 2.0, 1.0, 1.0
    for k, v in over.items():
        setattr(p, k, v)
    return p


def sense_params(**over):
    s = _lib.SenseParams()
    s.n_unknown, s.persistent, s.att_type = 3, 1, _lib.ATT_VELOCITY_TRACKING_YAW
    s.fov_angle, s.cam_range, s.w_max = np.deg2rad(70.0), 3.0, 0.5
    s.att_kp, s.att_preview_time, s.simple_yaw_rate = 1.5, 0.0, 0.5
    for k, v in over.items():
        setattr(s, k, v)
    return s


def test_symbol_version_and_constants():
    lib = _lib.load()
    fn = lib.sc_tracking_sense_rollout_batch
    assert "sc_tracking_sense_rollout_batch" in _lib.SYMBOLS and len(fn.argtypes) == 23
    assert fn.argtypes[0] == C.POINTER(_lib.TrackingParams) and fn.argtypes[1] == C.POINTER(_lib.SenseParams)
    assert lib.sc_version() == 9 and _lib.ABI_VERSION == 9                  # additive: the version does not move
    assert (_lib.ATT_NONE, _lib.ATT_SIMPLE, _lib.ATT_VELOCITY_TRACKING_YAW, _lib.SENSE_MAX_UNKNOWN) == (0, 1, 2, 64)


def test_header_struct_matches_the_mirror(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safe_control_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(sc_sense_params), sizeof(sc_tracking_params),\n'
                   '         offsetof(sc_sense_params, att_type), offsetof(sc_sense_params, fov_angle), offsetof(sc_sense_params, simple_yaw_rate),\n'
                   '         SC_ATT_NONE, SC_ATT_SIMPLE, SC_ATT_VELOCITY_TRACKING_YAW, SC_SENSE_MAX_UNKNOWN);\n  return 0;\n}\n')
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    S = _lib.SenseParams
    assert got == [C.sizeof(S), C.sizeof(_lib.TrackingParams), S.att_type.offset, S.fov_angle.offset, S.simple_yaw_rate.offset,
                   _lib.ATT_NONE, _lib.ATT_SIMPLE, _lib.ATT_VELOCITY_TRACKING_YAW, _lib.SENSE_MAX_UNKNOWN]
    assert C.sizeof(S) == 64


def test_argument_validation_without_gpu():
    lib = _lib.load()
    ptr = np.zeros(4096).ctypes.data
    iptr = np.zeros(64, dtype=np.int64).ctypes.data

    def call(p, s, B=1, M=1, unknown=ptr, seen=iptr, yaw=ptr, u_att=ptr, X=ptr):
        return lib.sc_tracking_sense_rollout_batch(
            C.byref(p) if p is not None else None, C.byref(s) if s is not None else None, B, M, X, ptr, iptr, iptr, iptr, ptr, ptr,
            unknown, seen, yaw, u_att, ptr, iptr, iptr, None, None, None, None, None)

    p, s = tracking_params(), sense_params()
    assert call(p, s, B=0) == OK                                           # every check passes; nothing to launch
    assert call(None, s) == INVALID and call(p, None) == INVALID and call(p, s, B=-1) == INVALID and call(p, s, M=-1) == INVALID
    # n_unknown in [0, 64], and a table when it is > 0
    assert call(p, sense_params(n_unknown=-1), B=0) == INVALID and call(p, sense_params(n_unknown=65), B=0) == INVALID
    assert call(p, sense_params(n_unknown=64), B=0) == OK and call(p, sense_params(n_unknown=0), B=0, unknown=None) == OK
    assert call(p, s, B=0, unknown=None) == INVALID
    assert call(p, s, B=0, seen=None) == INVALID
    # static tables, at least one step, 1..16 constraints
    assert call(tracking_params(dyn_obs=1), s, B=0) == UNSUPPORTED
    assert call(tracking_params(n_steps=0), s, B=0) == INVALID
    assert call(tracking_params(num_constraints=0), s, B=0) == UNSUPPORTED and call(tracking_params(num_constraints=17), s, B=0) == UNSUPPORTED
    assert call(tracking_params(num_constraints=16), s, B=0) == OK
    # models
    for model in ("KinematicBicycle2D", "Unicycle2D", "KinematicBicycle2D_C3BF"):
        assert call(tracking_params(model), sense_params(att_type=_lib.ATT_NONE), B=0) == UNSUPPORTED, model
    du = tracking_params("DynamicUnicycle2D")
    assert call(du, sense_params(att_type=_lib.ATT_NONE), B=0, yaw=None, u_att=None) == OK
    assert call(du, sense_params(att_type=_lib.ATT_SIMPLE), B=0) == INVALID     # an attitude controller belongs to the integrators
    assert call(p, sense_params(att_type=3), B=0) == INVALID
    # a rotating integrator needs a controller and its two arrays; a non-rotating one does not
    for model in ("SingleIntegrator2D", "DoubleIntegrator2D"):
        q = tracking_params(model)
        assert call(q, sense_params(att_type=_lib.ATT_NONE), B=0) == INVALID, model
        assert call(q, s, B=0, yaw=None) == INVALID and call(q, s, B=0, u_att=None) == INVALID, model
        assert call(q, sense_params(att_type=_lib.ATT_SIMPLE), B=0) == OK, model
        q0 = tracking_params(model, enable_rotation=0)
        assert call(q0, sense_params(att_type=_lib.ATT_NONE), B=0, yaw=None, u_att=None) == OK, model
    # the camera and the yaw-rate bound
    for field in ("fov_angle", "cam_range", "w_max"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert call(p, sense_params(**{field: bad}), B=0) == INVALID, (field, bad)
    assert call(p, s, X=None) == INVALID                                    # B > 0 with a NULL state array
    msg = lib.sc_last_error()
    assert msg and b"NULL" in msg


def test_controller_checks_its_arguments_before_any_device_tensor(monkeypatch):
    import torch

    def no_device(*a, **k):
        raise AssertionError("a device tensor was created before the arguments were checked")

    for name in ("tensor", "zeros", "full", "empty"):
        monkeypatch.setattr(torch, name, no_device)
    T = sca.BatchedSensingTrackingController
    di = {"model": "DoubleIntegrator2D", "radius": 0.25}
    x_di, x_du = np.array([[2.0, 2.0, 0.0, 0.0, 0.0]]), np.array([[2.0, 2.0, 0.0]])
    with pytest.raises(ValueError, match="supports"):
        T(x_du, {"model": "KinematicBicycle2D"})
    with pytest.raises(ValueError, match="cbf_qp"):
        T(x_di, di, controller_type={"pos": "mpc_cbf"})
    for att in ("visibility_raycast", "visibility_area", "gatekeeper"):
        with pytest.raises(ValueError, match="polygon geometry"):
            T(x_di, di, controller_type={"pos": "cbf_qp", "att": att})
    with pytest.raises(ValueError, match="attitude controller"):
        T(x_di, di, controller_type={"att": "pid"})
    with pytest.raises(ValueError, match="ray"):
        T(x_di, dict(di, unknown_obs_detection="ray"))
    with pytest.raises(ValueError, match="unknown_obs_detection"):
        T(x_di, dict(di, unknown_obs_detection="lidar"))
    with pytest.raises(ValueError, match="at most 64"):
        T(x_di, di, unknown_obs=[[float(i), 20.0, 0.2] for i in range(65)])
    with pytest.raises(ValueError, match="one obstacle"):
        T(x_di, di, unknown_obs=[[5.0, 5.0, 0.4], [8.0, 8.0, 0.3], [5.0005, 5.0, 0.405]])
    with pytest.raises(ValueError, match="one obstacle"):                    # a superellipsoid is remembered as its outer circle
        T(x_di, di, unknown_obs=[[5.0, 5.0, 0.6, 0, 0, 0, 0], [5.0, 5.0, 0.3, 0.6, 2, 0.3, 1]])
    with pytest.raises(ValueError, match="num_constraints"):
        T(x_di, dict(di, num_constraints=17))
    for key in ("fov_angle", "cam_range", "w_max"):
        with pytest.raises(ValueError, match=key):
            T(x_di, dict(di, **{key: 0.0}))
    with pytest.raises(ValueError, match="io_dtype"):
        T(x_di, di, io_dtype="f16")
    # the base class is as it was: it has no attitude controller to turn an integrator with
    with pytest.raises(ValueError):
        sca.BatchedTrackingController(x_di, di, obs=np.array([[4.0, 3.5, 0.6]]))
    with pytest.raises(ValueError):
        sca.BatchedTrackingController(np.array([[2.0, 2.0, 0.0]]), {"model": "SingleIntegrator2D"}, obs=np.array([[4.0, 3.5, 0.6]]))


def test_unknown_rows_are_normalised_like_the_reference():
    T = sca.BatchedSensingTrackingController
    self = T.__new__(T, None, {"model": "DoubleIntegrator2D"})
    self.merge_tol, self.merge_radius_tol = 1e-3, 1e-2
    u = self._normalise_unknown([[1.0, 2.0, 0.3], [4.0, 5.0, 0.2]])           # tracking.py:283-285
    assert u.shape == (2, 7) and np.array_equal(u[:, 3:], np.zeros((2, 4))) and np.array_equal(u[:, :3], [[1, 2, .3], [4, 5, .2]])
    assert self._normalise_unknown([1.0, 2.0, 0.3, 0.1, 2.0]).shape == (1, 7)   # one short row (:279-280, :286-288)
    assert np.array_equal(self._normalise_unknown([[1.0, 2.0, 0.3, 0.6, 2.0, 0.3, 1.0, 9.0, 9.0]]), [[1.0, 2.0, 0.3, 0.6, 2.0, 0.3, 1.0]])
    assert self._normalise_unknown(None).shape == (0, 7) and self._normalise_unknown([]).shape == (0, 7)
    assert self._normalise_unknown([[float(i), 20.0, 0.2] for i in range(64)]).shape == (64, 7)
