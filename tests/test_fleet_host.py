"""Host tests of the fleet closed loop: argument checks of sc_tracking_fleet_step_batch (no GPU is touched: every argument is
checked before the first HIP call), the fleet oracle against per-agent TrackingOracle runs and the brute-force neighbour
search, and the fleet scene."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _fleet_oracle as FO  # noqa: E402
from oracle import robots as R  # noqa: E402
from oracle.tracking import TrackingOracle  # noqa: E402
from safe_control_amd import _lib, workloads as W  # noqa: E402
from safe_control_amd.position_control.cbf_qp import default_cbf_param, make_params  # noqa: E402
from safe_control_amd.robots.spec import complete_robot_spec  # noqa: E402


def _params(model="KinematicBicycle2D_C3BF", n_steps=1, io=_lib.DTYPE_F64):
    rs = complete_robot_spec({"model": model})
    p = _lib.TrackingParams()
    p.qp = make_params(rs, default_cbf_param(model), 0.05, rs["radius"], io, _lib.DTYPE_F64)
    p.n_steps = n_steps
    p.max_waypoints = 1
    p.enable_rotation = 1
    p.dyn_obs = 1
    p.num_constraints = 10
    p.reached_threshold, p.rotation_threshold = 0.3, 0.1
    p.v_max, p.v_min = float(rs["v_max"]), float(rs.get("v_min", 0.0))
    p.k_omega, p.k_a, p.k_v = 2.0, 1.0, 1.0
    p.delta_max, p.wheel_base = float(rs.get("delta_max", 0.0)), float(rs.get("wheel_base", 0.0))
    return p


def _call(p, B=4, M=8, K=16, step=0, null=None):
    """Fake (never dereferenced) non-NULL addresses for every array, or NULL for the one named ``null``."""
    names = ["X", "X_pub", "waypoints", "n_wp", "wp_index", "state_machine", "goal", "obs_table", "nb_rows", "u_last", "ret",
             "ret_step", "cause", "min_sep"]
    ptrs = [None if n == null else 0x1000 * (i + 1) for i, n in enumerate(names)]
    lib = _lib.load()
    return lib.sc_tracking_fleet_step_batch(C.byref(p) if p is not None else None, B, M, K, step, *ptrs, None)


def test_fleet_entry_point_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.sc_version() >= 9
    assert _call(None) == _lib.SC_ERR_INVALID_ARGUMENT
    for name in ["X", "X_pub", "waypoints", "n_wp", "wp_index", "state_machine", "goal", "obs_table", "nb_rows", "u_last", "ret",
                 "ret_step", "cause", "min_sep"]:
        assert _call(_params(), null=name) == _lib.SC_ERR_INVALID_ARGUMENT, name
    assert _call(_params(), B=0) == _lib.SC_OK                            # nothing to do: no launch
    assert _call(_params(), K=33) == _lib.SC_ERR_UNSUPPORTED
    assert _call(_params(), M=33, K=0) == _lib.SC_ERR_UNSUPPORTED
    assert _call(_params(), M=33, K=32) == _lib.SC_ERR_UNSUPPORTED        # M + K_nb > 64 (each limit alone keeps it <= 64)
    assert _call(_params(), K=-1) == _lib.SC_ERR_INVALID_ARGUMENT
    assert _call(_params(), step=-1) == _lib.SC_ERR_INVALID_ARGUMENT
    assert _call(_params(n_steps=2)) == _lib.SC_ERR_INVALID_ARGUMENT
    assert b"n_steps" in lib.sc_last_error()
    assert _call(_params(n_steps=0)) == _lib.SC_ERR_INVALID_ARGUMENT
    for model in ("Unicycle2D", "SingleIntegrator2D", "DoubleIntegrator2D"):
        assert _call(_params(model)) == _lib.SC_ERR_UNSUPPORTED, model
    p = _params(); p.qp.model_id = 99
    assert _call(p) == _lib.SC_ERR_UNSUPPORTED
    p = _params(); p.num_constraints = 17
    assert _call(p) == _lib.SC_ERR_UNSUPPORTED
    p = _params(); p.qp.io_dtype = 7
    assert _call(p) == _lib.SC_ERR_INVALID_ARGUMENT


def test_fleet_class_rejects_unsupported_configurations():
    from safe_control_amd.tracking import BatchedFleetTrackingController as F
    X0 = np.zeros((4, 4))
    with pytest.raises(ValueError):
        F(X0, {"model": "Unicycle2D"})
    with pytest.raises(ValueError):
        F(X0, {"model": "KinematicBicycle2D_C3BF"}, controller_type={"pos": "mpc_cbf"})
    with pytest.raises(ValueError):
        F(X0, {"model": "KinematicBicycle2D_C3BF"}, neighbours=33)
    with pytest.raises(ValueError):
        F(X0, {"model": "KinematicBicycle2D_C3BF"}, obs=np.zeros((33, 7)), neighbours=0)
    with pytest.raises(ValueError):
        F(X0, {"model": "KinematicBicycle2D_C3BF"}, num_constraints=17)
    sup = np.zeros((1, 7)); sup[0, 6] = 1.0
    with pytest.raises(ValueError):
        F(X0, {"model": "DynamicUnicycle2D"}, obs=sup)


def test_fleet_oracle_without_neighbours_is_the_single_agent_oracle():
    """K_nb = 0: every agent runs TrackingOracle(dyn_obs=True) against its own copy of the moving table."""
    X0, wps, obs = W.kb_c3bf_fleet_scene(6, 4, seed=2)
    spec = {"model": "KinematicBicycle2D_C3BF"}
    fo = FO.FleetOracle("KinematicBicycle2D_C3BF", X0, spec, wps, obs=obs, dyn_obs=True, K_nb=0)
    T = 60
    for _ in range(T):
        fo.step()
    for i in range(len(X0)):
        t = TrackingOracle(R.MODEL_KB_C3BF, X0[i], {}, dt=0.05, obs=obs, dyn_obs=True)
        t.set_waypoints(wps[i])
        ret = 0
        for k in range(T):
            ret = t.control_step()
            if ret != 0:
                assert fo.ret[i] == ret and fo.ret_step[i] == k
                break
        if ret == 0:
            assert fo.ret[i] == 0
        np.testing.assert_array_equal(fo.agents[i].X, t.X)
    assert np.isinf(fo.min_sep).all()


def test_fleet_oracle_neighbours_are_the_brute_force_search():
    """N_i equals tests/test_neighbors_gpu.py's brute force (radius as the kernel stores it, no padding rows)."""
    rng = np.random.default_rng(4)
    for n, K in ((300, 16), (9, 16), (50, 32)):
        P = np.column_stack([rng.uniform(0, 20, n), rng.uniform(0, 20, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(0, 3, n)])
        P[1, :2] = P[0, :2] + 1.0; P[2, :2] = P[0, :2] - 1.0             # a tie: two agents at the same distance from agent 0
        rows = FO.neighbour_rows(P, K, 0.3)
        r = float(np.float32(0.3))
        for i in range(n):
            d = (P[:, 0] - P[i, 0]) ** 2 + (P[:, 1] - P[i, 1]) ** 2
            d[i] = np.inf
            idx = np.argsort(d, kind="stable")[: min(K, n - 1)]
            want = np.array([[P[j, 0], P[j, 1], r, P[j, 3] * np.cos(P[j, 2]), P[j, 3] * np.sin(P[j, 2]), 0, 0] for j in idx])
            np.testing.assert_array_equal(rows[i], want)
        xs = list(rows[0][:, 0])
        assert xs.index(P[2, 0]) == xs.index(P[1, 0]) + 1                 # ties: lower index first


def test_fleet_scene_starts_clear():
    for n in (96, 1000):
        X0, wps, obs = W.kb_c3bf_fleet_scene(n, 16, seed=1)
        R_ = complete_robot_spec({"model": "KinematicBicycle2D_C3BF"})["radius"]
        d = np.hypot(X0[:, None, 0] - X0[None, :, 0], X0[:, None, 1] - X0[None, :, 1]) + np.eye(n) * 1e9
        assert d.min() > 2 * R_ + 1.0
        do = np.hypot(X0[:, None, 0] - obs[None, :, 0], X0[:, None, 1] - obs[None, :, 1])
        assert do.min() > 0.5 + R_
        gd = np.hypot(wps[:, 0, 0] - X0[:, 0], wps[:, 0, 1] - X0[:, 1])
        assert gd.min() >= 10.0 and gd.max() <= 20.0
        ang = np.arctan2(wps[:, 0, 1] - X0[:, 1], wps[:, 0, 0] - X0[:, 0])
        np.testing.assert_allclose(np.cos(ang - X0[:, 2]), 1.0, atol=1e-12)
        assert (X0[:, 3] > 0).all() and (obs[:, 2] == 0.5).all() and (np.abs(obs[:, 3:5]) <= 0.5).all()
