"""CPU: the Quad2D closed-loop entry point (sc_tracking_quad2d_rollout_batch) exists with its argument types, sc_tracking_quad2d_params
compiles as C99 with the size and offsets of the ctypes mirror, the ABI version is unchanged (the addition is additive) and every
documented refusal returns its code before any HIP call."""
import ctypes as C
import os
import subprocess

import numpy as np

from safe_control_amd import _lib
from safe_control_amd.position_control.cbf_qp import default_cbf_param, make_params
from safe_control_amd.position_control.optimal_decay_cbf_qp import default_od_param
from safe_control_amd.robots.spec import complete_robot_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = _lib.SC_ERR_INVALID_ARGUMENT, _lib.SC_ERR_UNSUPPORTED
CBF, OD = _lib.QUAD2D_CTRL_CBF_QP, _lib.QUAD2D_CTRL_OD_CBF_QP


def params(controller=CBF, n_steps=3):
    rs = complete_robot_spec({"model": "Quad2D"})
    p = _lib.TrackingQuad2dParams()
    t = p.od.track
    prm = default_od_param("Quad2D") if controller == OD else default_cbf_param("Quad2D")
    t.qp = make_params(rs, prm, 0.05, rs["radius"], _lib.DTYPE_F64, _lib.DTYPE_F64)
    t.n_steps, t.max_waypoints, t.num_constraints = n_steps, 2, 3
    t.reached_threshold, t.rotation_threshold = 0.3, 0.1
    p.od.omega_ref[0] = p.od.omega_ref[1] = 1.0
    p.od.p_sb[0] = p.od.p_sb[1] = 1e4
    p.controller = controller
    p.inertia = float(rs["inertia"])
    return p


def test_symbol_version_and_signature():
    lib = _lib.load()
    assert lib.sc_version() == 9 == _lib.ABI_VERSION
    fn = lib.sc_tracking_quad2d_rollout_batch
    assert fn.argtypes[0] == C.POINTER(_lib.TrackingQuad2dParams) and fn.argtypes[1:3] == [C.c_int64, C.c_int32]
    assert fn.argtypes[3:] == [C.c_void_p] * 16 and fn.restype == C.c_int
    p = params()
    assert p.od.track.qp.model_id == _lib.MODEL_IDS["Quad2D"] and p.od.track.qp.state_dim == 6
    assert (p.od.track.qp.u_min[0], p.od.track.qp.u_max[1]) == (1.0, 10.0)          # the thrust box [f_min, f_max]^2


def test_header_struct_matches_the_mirror(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safe_control_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(sc_tracking_quad2d_params), sizeof(sc_tracking_od_params),\n'
                   '         offsetof(sc_tracking_quad2d_params, od), offsetof(sc_tracking_quad2d_params, controller),\n'
                   '         offsetof(sc_tracking_quad2d_params, reserved0), offsetof(sc_tracking_quad2d_params, inertia),\n'
                   '         SC_QUAD2D_CTRL_CBF_QP, SC_QUAD2D_CTRL_OD_CBF_QP);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    S = _lib.TrackingQuad2dParams
    assert got == [C.sizeof(S), C.sizeof(_lib.TrackingOdParams), S.od.offset, S.controller.offset, S.reserved0.offset, S.inertia.offset,
                   CBF, OD]
    assert C.sizeof(S) == C.sizeof(_lib.TrackingOdParams) + 16


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
        return lib.sc_tracking_quad2d_rollout_batch(C.byref(p) if p is not None else None, B, M, *[a[n] for n in names], None)

    assert call(None) == INVALID
    for ctrl in (CBF, OD):
        p = params(ctrl)
        assert call(p, B=-1) == INVALID and call(p, M=-1) == INVALID
        for required in ("X", "waypoints", "n_wp", "wp_index", "state_machine", "goal", "u_last", "ret", "ret_step"):
            assert call(p, **{required: None}) == INVALID, (ctrl, required)
        assert call(p, M=2, obs_table=None) == INVALID                           # M without a table
        for model in _lib.MODEL_IDS:                                             # a model other than Quad2D
            if model != "Quad2D":
                q = params(ctrl); q.od.track.qp.model_id = _lib.MODEL_IDS[model]
                assert call(q) == UNSUPPORTED, model
        q = params(ctrl); q.od.track.qp.model_id = -1
        assert call(q) == UNSUPPORTED
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            q = params(ctrl); q.od.track.qp.mass = bad
            assert call(q) == INVALID, ("mass", bad)
            q = params(ctrl); q.inertia = bad
            assert call(q) == INVALID, ("inertia", bad)
            q = params(ctrl); q.od.track.qp.robot_radius = bad
            assert call(q) == INVALID, ("robot_radius", bad)
            q = params(ctrl); q.od.track.qp.dt = bad
            assert call(q) == INVALID, ("dt", bad)
        q = params(ctrl); q.od.track.qp.u_min[0] = 11.0                          # f_min > f_max
        assert call(q) == INVALID
        q = params(ctrl); q.od.track.qp.u_max[1] = 0.5
        assert call(q) == INVALID
        q = params(ctrl); q.od.track.qp.io_dtype = 7
        assert call(q) == INVALID
        q = params(ctrl); q.od.track.max_waypoints = 0
        assert call(q) == INVALID
        assert call(p, B=0, **{n: None for n in names}) == _lib.SC_OK           # B == 0 returns 0
        assert call(params(ctrl, n_steps=0)) == _lib.SC_OK
    for ctrl in (-1, 2, 7):                                                      # an unknown controller
        q = params(); q.controller = ctrl
        assert call(q) == UNSUPPORTED, ctrl
    # 'cbf_qp': num_constraints inside [1, SC_TRACKING_MAX_CONSTRAINTS]; omega / min_h / traj_omega are ignored and may be NULL
    for K in (0, -3, _lib.TRACKING_MAX_CONSTRAINTS + 1):
        q = params(CBF); q.od.track.num_constraints = K
        assert call(q) == INVALID, K
        q = params(OD); q.od.track.num_constraints = K                           # optimal decay takes the nearest row only
        assert call(q, B=0) == _lib.SC_OK, K
    q = params(CBF); q.od.p_sb[0] = 0.0                                          # read only under optimal decay
    assert call(q, B=0) == _lib.SC_OK
    assert call(params(CBF, n_steps=0), omega=None, min_h=None, traj_omega=None) == _lib.SC_OK
    # optimal decay: omega and min_h are required, p_sb positive
    for required in ("omega", "min_h"):
        assert call(params(OD), **{required: None}) == INVALID, required
    for i, bad in ((0, 0.0), (1, 0.0), (0, -1.0), (1, float("nan"))):
        q = params(OD); q.od.p_sb[i] = bad
        assert call(q) == INVALID, (i, bad)
