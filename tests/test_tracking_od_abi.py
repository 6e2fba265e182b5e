"""CPU: the optimal-decay closed-loop entry point (sc_tracking_od_rollout_batch) exists with its argument types, sc_tracking_od_params
compiles as C99 with the size and offsets of the ctypes mirror, the ABI version is unchanged (the addition is additive) and every
documented refusal returns its code before any HIP call."""
import ctypes as C
import os
import subprocess

import numpy as np

from safe_control_amd import _lib
from safe_control_amd.position_control.cbf_qp import make_params
from safe_control_amd.position_control.optimal_decay_cbf_qp import apply_od_overrides, default_od_param
from safe_control_amd.robots.spec import complete_robot_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = _lib.SC_ERR_INVALID_ARGUMENT, _lib.SC_ERR_UNSUPPORTED


def params(model="DynamicUnicycle2D", n_steps=3):
    rs = complete_robot_spec({"model": model})
    p = _lib.TrackingOdParams()
    p.track.qp = make_params(rs, default_od_param(model), 0.05, rs["radius"], _lib.DTYPE_F64, _lib.DTYPE_F64)
    p.track.n_steps, p.track.max_waypoints, p.track.num_constraints = n_steps, 2, 1
    p.track.reached_threshold, p.track.rotation_threshold = 0.3, 0.1
    p.track.v_max, p.track.v_min = float(rs["v_max"]), float(rs.get("v_min", 0.0))
    p.track.k_omega, p.track.k_a, p.track.k_v = 3.0, 0.5, 0.5
    p.track.delta_max, p.track.wheel_base = float(rs.get("delta_max", 0.0)), float(rs.get("wheel_base", 0.0))
    p.omega_ref[0] = p.omega_ref[1] = 1.0
    p.p_sb[0] = p.p_sb[1] = 1e4
    p.k_a_stop = 1.0
    return p


def test_symbol_version_and_signature():
    lib = _lib.load()
    assert lib.sc_version() == 9 == _lib.ABI_VERSION
    fn = lib.sc_tracking_od_rollout_batch
    assert fn.argtypes[0] == C.POINTER(_lib.TrackingOdParams) and fn.argtypes[1:3] == [C.c_int64, C.c_int32]
    assert len(fn.argtypes) == 19 and fn.restype == C.c_int


def test_header_struct_matches_the_mirror(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safe_control_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(sc_tracking_od_params), sizeof(sc_tracking_params),\n'
                   '         offsetof(sc_tracking_od_params, track), offsetof(sc_tracking_od_params, omega_ref),\n'
                   '         offsetof(sc_tracking_od_params, p_sb), offsetof(sc_tracking_od_params, k_a_stop),\n'
                   '         offsetof(sc_tracking_od_params, reserved));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    S = _lib.TrackingOdParams
    assert got == [C.sizeof(S), C.sizeof(_lib.TrackingParams), S.track.offset, S.omega_ref.offset, S.p_sb.offset, S.k_a_stop.offset,
                   S.reserved.offset]
    assert C.sizeof(S) == C.sizeof(_lib.TrackingParams) + 6 * 8


def test_refusals_need_no_gpu():
    lib = _lib.load()
    ptr = np.zeros(256).ctypes.data
    iptr = np.zeros(64, dtype=np.int32).ctypes.data
    names = ("X", "waypoints", "n_wp", "wp_index", "state_machine", "goal", "obs_table", "u_last", "ret", "ret_step", "traj_X", "traj_U",
             "omega", "min_h", "traj_omega")
    good = dict(X=ptr, waypoints=ptr, n_wp=iptr, wp_index=iptr, state_machine=iptr, goal=ptr, obs_table=ptr, u_last=ptr, ret=iptr,
                ret_step=iptr, traj_X=None, traj_U=None, omega=ptr, min_h=ptr, traj_omega=None)

    def call(p, B=1, M=1, **over):
        a = dict(good, **over)
        return lib.sc_tracking_od_rollout_batch(C.byref(p) if p is not None else None, B, M, *[a[n] for n in names], None)

    p = params()
    assert call(None) == INVALID and call(p, B=-1) == INVALID and call(p, M=-1) == INVALID
    for required in ("X", "waypoints", "n_wp", "wp_index", "state_machine", "goal", "u_last", "ret", "ret_step", "omega", "min_h"):
        assert call(p, **{required: None}) == INVALID, required
    assert call(p, M=2, obs_table=None) == INVALID                               # M without a table
    for model in ("SingleIntegrator2D", "DoubleIntegrator2D", "Quad2D", "Unicycle2D"):
        q = params()
        q.track.qp.model_id = _lib.MODEL_IDS[model]
        assert call(q) == UNSUPPORTED, model
    q = params(); q.track.qp.model_id = -1
    assert call(q) == UNSUPPORTED
    for i, bad in ((0, 0.0), (1, 0.0), (0, -1.0), (1, float("nan"))):
        q = params(); q.p_sb[i] = bad
        assert call(q) == INVALID, (i, bad)
    for model in ("KinematicBicycle2D", "KinematicBicycle2D_C3BF", "KinematicBicycle2D_DPCBF"):
        q = params(model); q.track.qp.rear_ax_dist = 0.0
        assert call(q) == INVALID, model
        q = params(model); q.track.wheel_base = 0.0
        assert call(q) == INVALID, model
    q = params(); q.track.qp.io_dtype = 7
    assert call(q) == INVALID
    q = params(); q.track.qp.dt = 0.0
    assert call(q) == INVALID
    q = params(); q.track.max_waypoints = 0
    assert call(q) == INVALID
    assert call(p, B=0, **{n: None for n in names}) == _lib.SC_OK               # B == 0 returns 0
    assert call(params(n_steps=0)) == _lib.SC_OK


def test_parameter_overrides_reach_the_decay_terms():
    """robot_spec keys cbf_alpha*, cbf_omega1/2, cbf_p_sb1/2 override the model's optimal-decay parameter set, and only keys it has."""
    prm = apply_od_overrides(default_od_param("DynamicUnicycle2D"), {"cbf_alpha1": 0.7, "cbf_omega2": 0.9, "cbf_p_sb1": 1.0, "cbf_p_sb2": 2.0})
    assert prm == dict(alpha1=0.7, alpha2=0.5, omega1=1.0, p_sb1=1.0, omega2=0.9, p_sb2=2.0)
    prm = apply_od_overrides(default_od_param("KinematicBicycle2D_C3BF"), {"cbf_alpha": 0.3, "cbf_p_sb1": 5.0, "cbf_p_sb2": 2.0})
    assert prm == dict(alpha=0.3, omega1=1.0, p_sb1=5.0)
