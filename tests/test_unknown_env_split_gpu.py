"""GPU: the sensing loop under 'mpc_cbf' (csrc/tracking_sense_split.hip, BatchedSensingMPCTrackingController).

  1. without unknown rows the two new entry points are sc_tracking_select_batch / sc_tracking_apply_batch, bit for bit;
  2. sensing, memory, selection, attitude and collisions against the split oracle (tests/_unknown_env_split_oracle.py) on the fleet
     scene, with a CBF-QP standing in for the MPC on both sides (1e-7, the tolerance tests/test_unknown_env_gpu.py holds
     DoubleIntegrator2D to);
  3. three closed loops with the real MPC kernels against the split oracle with the matching MPC oracle behind solve_fn, at the
     tolerances tests/test_tracking_gpu.py allows the same models' MPC loops (5e-6 DynamicUnicycle2D and SingleIntegrator2D, 2e-5
     DoubleIntegrator2D);
  4. f32 storage, and a run cut into two launches.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import safe_control_amd as sca  # noqa: E402
from safe_control_amd import _lib  # noqa: E402
import _unknown_env_oracle as O  # noqa: E402
import _unknown_env_split_oracle as S  # noqa: E402

pytestmark = pytest.mark.gpu


def cpu(t):
    return t.detach().cpu().numpy()


def u64(t):
    return cpu(t).view(np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. Mu = 0 is the plain split ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_constraints", [5, 10])                         # KMAX 8 and 16
@pytest.mark.parametrize("model", ["DynamicUnicycle2D", "DoubleIntegrator2D"])
def test_no_unknown_rows_is_the_plain_split_bit_for_bit(golden_dir, model, num_constraints):
    rng = np.random.default_rng(11)
    B, T = 130, 20                                                           # two blocks and a two-lane tail
    if model == "DynamicUnicycle2D":
        g = np.load(os.path.join(golden_dir, "closed_loop.npz"))
        obs, wps = g["du14/obs"], g["du14/waypoints"]
        spec, rot = {"model": model, "a_max": 1.0, "w_max": 0.5, "radius": 0.25}, True
        X0 = np.column_stack([2.0 + rng.uniform(-0.4, 0.4, (B, 2)), rng.uniform(-np.pi, np.pi, B), rng.uniform(0, 1, B)])
    else:
        g = np.load(os.path.join(golden_dir, "closed_loop_integrators.npz"))
        obs, wps = g["di/obs"], g["di/waypoints"]
        spec, rot = {"model": model, "v_max": 1.0, "a_max": 1.0, "radius": 0.25}, False
        X0 = np.column_stack([2.0 + rng.uniform(-0.4, 0.4, (B, 2)), rng.uniform(-0.3, 0.3, (B, 2)), rng.uniform(-np.pi, np.pi, B)])
    spec["num_constraints"] = num_constraints
    mpc = {"pos": "mpc_cbf"}
    base = sca.BatchedTrackingController(X0, dict(spec), controller_type=mpc, enable_rotation=rot, obs=obs)
    new = sca.BatchedSensingMPCTrackingController(X0, dict(spec), controller_type=mpc, enable_rotation=rot, obs=obs, unknown_obs=None)
    assert new.unknown_obs.shape[0] == 0 and new.att_type == _lib.ATT_NONE
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    M = int(base.obs.shape[0])
    outs = {}
    for name, c in (("base", base), ("new", new)):
        c.set_waypoints(wps)
        new_t = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=c.device)
        outs[name] = dict(obs_out=new_t((B, num_constraints, 7)), goal_out=new_t((B, 2)), u_ref_out=new_t((B, 2)),
                          track_out=new_t((B,), torch.int32))
    pb, pn, sn = base._split_params(), new._split_params(), new._sense_params()
    lo = torch.tensor([pb.qp.u_min[0], pb.qp.u_min[1]], dtype=torch.float64, device=base.device)
    hi = torch.tensor([pb.qp.u_max[0], pb.qp.u_max[1]], dtype=torch.float64, device=base.device)
    seen_track = seen_other = False
    for k in range(T):
        ob, on = outs["base"], outs["new"]
        rc = lib.sc_tracking_select_batch(
            C.byref(pb), B, M, base.X.data_ptr(), base.waypoints.data_ptr(), base.n_wp.data_ptr(), base.current_goal_index.data_ptr(),
            base.state_machine.data_ptr(), base.goal.data_ptr(), base.obs.data_ptr(), base.ret.data_ptr(), ob["obs_out"].data_ptr(),
            ob["goal_out"].data_ptr(), ob["u_ref_out"].data_ptr(), ob["track_out"].data_ptr(), stream)
        _lib.check(rc, "sc_tracking_select_batch")
        rc = lib.sc_tracking_sense_select_batch(
            C.byref(pn), C.byref(sn), B, M, new.X.data_ptr(), new.waypoints.data_ptr(), new.n_wp.data_ptr(),
            new.current_goal_index.data_ptr(), new.state_machine.data_ptr(), new.goal.data_ptr(), new.obs.data_ptr(), None,
            new.seen.data_ptr(), new.yaw.data_ptr(), new.u_att.data_ptr(), new.ret.data_ptr(), on["obs_out"].data_ptr(),
            on["goal_out"].data_ptr(), on["u_ref_out"].data_ptr(), on["track_out"].data_ptr(), stream)
        _lib.check(rc, "sc_tracking_sense_select_batch")
        for name in ("obs_out", "goal_out", "u_ref_out", "track_out"):
            assert same_bits(cpu(ob[name]), cpu(on[name])), f"step {k}: {name}"
        for name in ("state_machine", "goal", "current_goal_index"):
            assert same_bits(cpu(getattr(base, name)), cpu(getattr(new, name))), f"step {k}: {name} after select"
        tr = cpu(ob["track_out"])
        seen_track |= bool((tr == 1).any())
        seen_other |= bool((tr == 0).any())
        u = torch.minimum(torch.maximum(ob["u_ref_out"], lo), hi).contiguous()      # the same stand-in input for both
        rc = lib.sc_tracking_apply_batch(
            C.byref(pb), B, M, k, base.X.data_ptr(), base.state_machine.data_ptr(), base.goal.data_ptr(), base.obs.data_ptr(),
            u.data_ptr(), None, base.u_pos.data_ptr(), base.ret.data_ptr(), base.ret_step.data_ptr(), stream)
        _lib.check(rc, "sc_tracking_apply_batch")
        rc = lib.sc_tracking_sense_apply_batch(
            C.byref(pn), C.byref(sn), B, M, k, new.X.data_ptr(), new.state_machine.data_ptr(), new.goal.data_ptr(), new.obs.data_ptr(),
            None, new.yaw.data_ptr(), new.u_att.data_ptr(), u.data_ptr(), None, new.u_pos.data_ptr(), new.ret.data_ptr(),
            new.ret_step.data_ptr(), stream)
        _lib.check(rc, "sc_tracking_sense_apply_batch")
        for name in ("X", "u_pos", "state_machine", "goal", "current_goal_index", "ret", "ret_step"):
            assert same_bits(cpu(getattr(base, name)), cpu(getattr(new, name))), f"step {k}: {name} after apply"
    assert seen_track and seen_other                                          # both kinds of agents were in the batch
    assert int(new.seen.abs().sum()) == 0
    assert np.linalg.norm(cpu(new.X)[:, :2] - X0[:, :2], axis=1).max() > 0.3


# ---- 2. sensing without the MPC's cost ------------------------------------------------------------------------------------------------
def fleet_controller(num_constraints, io_dtype="f64", stand_in=True, monkeypatch=None, round32=False):
    sc = S.fleet_split_scene()
    f = (lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)) if round32 else (lambda a: a)   # inputs both storages hold exactly
    spec = dict(O.FLEET_SPEC, model="DoubleIntegrator2D", num_constraints=num_constraints)
    ctl = sca.BatchedSensingMPCTrackingController(f(sc["X0"]), spec, controller_type={"pos": "mpc_cbf", "att": "velocity_tracking_yaw"},
                                                  obs=f(sc["obs"]), unknown_obs=f(sc["unknown"]), io_dtype=io_dtype)
    ctl.set_waypoints(f(sc["waypoints"]))
    if stand_in:
        qp = sca.BatchedCBFQP(dict(spec), io_dtype=io_dtype, compute_dtype="f64")
        zeros = torch.zeros(ctl.B, dtype=torch.int32, device=ctl.device)

        class StandIn:
            """The batched CBF-QP on the rows the controller was shown; a QP without a solution hands u_ref on."""
            def solve(self, X_in, up_in, goal_in, obs_in):
                u, st, _ = qp.solve(X_in, ctl.u_ref, ctl.obs_sel)
                return torch.where((st == 0).unsqueeze(1), u, ctl.u_ref).contiguous(), zeros, zeros

        monkeypatch.setattr(ctl, "_split_solver", lambda: StandIn())
    return ctl


@pytest.mark.parametrize("num_constraints", [10, 5])                        # KMAX 16 and 8
def test_sensing_against_the_split_oracle(monkeypatch, num_constraints):
    ref = S.fleet_split_oracle(num_constraints)
    ctl = fleet_controller(num_constraints, monkeypatch=monkeypatch)
    assert ctl.B == 130 and ctl.unknown_obs.shape[0] == 33 and ctl.obs.shape[0] == 12
    ret, tX, tU, tY, tS = ctl.control_step(S.FLEET_SPLIT_STEPS, record=True)
    tX, tU, tY, tS, ret, rstep, sm = cpu(tX), cpu(tU), cpu(tY), u64(tS), cpu(ret), cpu(ctl.ret_step), cpu(ctl.state_machine)
    excluded, worst = [], 0.0
    for i, r in enumerate(ref):
        if float(r["min_margin"]) < 1e-6:                                    # a sighting decided by less than the comparison's tolerance
            excluded.append(i)
            continue
        n = len(r["ret"])
        worst = max(worst, np.abs(tX[:n, i] - r["X"]).max(), np.abs(tU[:n, i] - r["U"]).max(), np.abs(tY[:n, i] - r["yaw"]).max())
    print(f"num_constraints {num_constraints}: excluded {excluded}, max deviation from the split oracle {worst:.2e}")
    assert len(excluded) <= 2
    for i, r in enumerate(ref):
        if i in excluded:
            continue
        n = len(r["ret"])
        np.testing.assert_allclose(tX[:n, i], r["X"], rtol=1e-7, atol=1e-7, err_msg=f"agent {i}")
        np.testing.assert_allclose(tU[:n, i], r["U"], rtol=1e-7, atol=1e-7, err_msg=f"agent {i}")
        np.testing.assert_allclose(tY[:n, i], r["yaw"], rtol=1e-7, atol=1e-7, err_msg=f"agent {i}")
        assert np.array_equal(tS[:n, i], r["mask"]), f"agent {i}: sighted rows"
        last = int(r["ret"][-1])
        assert ret[i] == last and rstep[i] == (n - 1 if last != 0 else -1) and sm[i] == r["sm"][-1], f"agent {i}"
    last_mask = tS[-1]
    assert (last_mask >> np.uint64(32)).astype(bool).any() and (last_mask & np.uint64(0xFFFFFFFF)).astype(bool).any()


@pytest.mark.parametrize("io", ["f64", "f32"])
@pytest.mark.parametrize("big", [False, True], ids=["m3", "m1171"])
@pytest.mark.parametrize("num_constraints", [8, 9])                         # KMAX 8 and 16
@pytest.mark.parametrize("name", sca.BatchedSensingMPCTrackingController.MODELS)
def test_every_kernel_of_the_sensing_select_and_apply_launchers(monkeypatch, name, num_constraints, big, io):
    """tracking_sense_select_kernel (KMAX 8 and 16) and tracking_sense_apply_kernel for their three models and both storage types, in
    the loop they serve with the batched CBF-QP standing in for the MPC (as above): 65 agents x 10 steps on three known and five
    unknown circles, and 3 agents x 2 steps on a known table of 1171 rows (65 576 B of LDS: the raised dynamic-LDS limit), against
    the split oracle.  f64: 1e-7, the figure of the test above.  f32: the loop stores state and heading as f32 after every step, at
    most 2^-24 * 16 = 9.5e-7 per step on values below 16; over n <= 10 steps these add up and pass through dynamics whose step
    Jacobian is 1 + O(dt), allowed for by a factor 2: 1e-7 + 2 n 9.5e-7."""
    import _agent_params_cases as AC
    T = AC.BIG_T if big else AC.RUNG_T
    case = AC.rung_case(name, False, big)
    spec = dict(case["specs"][0], num_constraints=num_constraints)
    ctl = sca.BatchedSensingMPCTrackingController(case["X0"], dict(spec), controller_type={"pos": "mpc_cbf", "att": "velocity_tracking_yaw"},
                                                  obs=case["obs"], unknown_obs=O.RUNG_UNKNOWN, io_dtype=io)
    ctl.set_waypoints(case["wl"])
    qp = sca.BatchedCBFQP(dict(spec), io_dtype=io, compute_dtype="f64")
    zeros = torch.zeros(ctl.B, dtype=torch.int32, device=ctl.device)

    class StandIn:
        def solve(self, X_in, up_in, goal_in, obs_in):
            u, st, _ = qp.solve(ctl.X, ctl.u_ref, ctl.obs_sel)
            return torch.where((st == 0).unsqueeze(1), u, ctl.u_ref).contiguous(), zeros, zeros

    monkeypatch.setattr(ctl, "_split_solver", lambda: StandIn())
    ret, tX, tU, tY, tS = ctl.control_step(T, record=True)

    def make(*a, **k):
        o = S.UnknownEnvSplitOracle(*a, solve_fn=lambda *x: None, **k)
        o.split_solve_fn = S.padded_cbf_qp_solve_fn(o)
        return o
    ref = O.rung_records(case, T, num_constraints, make)
    O.assert_records(ref, cpu(tX.double()), cpu(tU.double()), cpu(tY.double()), u64(tS), cpu(ret), cpu(ctl.ret_step), cpu(ctl.state_machine),
                     1e-7 + (2 * T * 16 * 2.0 ** -24 if io == "f32" else 0.0))


# ---- 3. the feature: closed loops with the MPC kernels ----------------------------------------------------------------------------
def feature_controller(sc, unknown=True, io_dtype="f64"):
    ctype = {"pos": "mpc_cbf"}
    if sc["att"] is not None:
        ctype["att"] = sc["att"]
    ctl = sca.BatchedSensingMPCTrackingController(sc["X0"], S.feature_robot_spec(sc), controller_type=ctype, obs=sc["obs"],
                                                  unknown_obs=sc["unknown"] if unknown else None, io_dtype=io_dtype)
    ctl.set_waypoints(S.FEATURE_WPS)
    return ctl


@pytest.mark.parametrize("tag", ["du", "di", "si"])
def test_closed_loop_with_mpc_against_the_split_oracle(tag):
    sc = S.FEATURE_SCENES[tag]
    T, tol = sc["steps"], sc["tol"]
    nx = 2 if tag == "si" else 4
    ctl = feature_controller(sc)
    if tag == "si":
        assert ctl.mpc_ms is None and type(ctl.mpc).__name__ == "BatchedLinearMPCCBF"
    else:
        assert ctl.mpc_ms is not None and ctl.mpc_ms.horizon == sc["horizon"]       # kernel 13 with the example's tuning
        assert ctl.mpc_ms.cbf_param["alpha1"] == sc["alpha"] == ctl.mpc_ms.cbf_param["alpha2"]
    sm0 = cpu(ctl.state_machine)
    assert (sm0[:2] == 1).all() and sm0[2] == 2                                 # the third agent faces away from its goal: 'stop'
    ret, tX, tU, tY, tS = ctl.control_step(T, record=True)
    tX, tY, tS, ret = cpu(tX), cpu(tY), u64(tS), cpu(ret)
    sel = cpu(ctl.obs_sel)
    assert sel.shape == (3, S.FEATURE_K, 7) and ctl.u_ref.shape == (3, 2) and ctl.track.shape == (3,)
    plain = feature_controller(sc, unknown=False)
    _, pX, _, _, pS = plain.control_step(T, record=True)
    pX = cpu(pX)
    assert int(cpu(pS).astype(np.int64).sum()) == 0
    n_solves, mid_run, worst = 0, 0, 0.0
    for i in range(3):
        o, state = S.feature_oracle(sc, i)
        r = O.run(o, T)
        n = len(r["ret"])
        dev = max(np.abs(tX[:n, i, :nx] - r["X"][:, :nx]).max(), np.abs(tY[:n, i] - r["yaw"]).max())
        worst = max(worst, dev)
        print(f"{tag} agent {i}: steps {n}, ret {int(r['ret'][-1])}, sighting margin {o.min_margin:.3e}, max |X, yaw - oracle| {dev:.2e}, "
              f"moved by the unknown rows {np.abs(tX[:, i] - pX[:, i]).max():.3e}, solves {state.get('n', 0)}")
        assert o.min_margin > 1e-3, f"agent {i}: a sighting decided by {o.min_margin}"
        np.testing.assert_allclose(tX[:n, i, :nx], r["X"][:, :nx], rtol=0, atol=tol, err_msg=f"agent {i}")
        np.testing.assert_allclose(tY[:n, i], r["yaw"], rtol=0, atol=tol, err_msg=f"agent {i}: yaw")
        assert np.array_equal(tS[:n, i], r["mask"]), f"agent {i}: sighted rows"
        last = int(r["ret"][-1])
        assert ret[i] == last and int(ctl.ret_step[i]) == (n - 1 if last != 0 else -1)
        assert int(ctl.state_machine[i]) == int(r["sm"][-1])
        n_solves += state.get("n", 0)
        first = [int(k) + 1 for k in np.flatnonzero(r["mask"][1:] != r["mask"][:-1])]
        if i < 2:                                                                # the two agents under way
            j = i                                                                # ... meet row i of the unknown table
            assert r["mask"][0] == 0 and len(first) == 1 and 0 < first[0] < n - 1 and int(r["mask"][-1]) == 1 << j, f"agent {i}: {first}"
            mid_run += 1
            want = O.seen_circle(sc["unknown"][j])                               # [x, y, r, 0, 0, 0, 0]: a superellipsoid as its outer circle
            assert any(np.array_equal(row, want) for row in sel[i]), f"agent {i}: row {j} is not among the rows its controller was shown"
            assert np.abs(tX[:, i] - pX[:, i]).max() > 1e-3, f"agent {i}: the sighted row does not move the trajectory"
            assert np.abs(tX[: first[0], i] - pX[: first[0], i]).max() == 0.0      # ... and nothing differs before it is sighted
    assert mid_run == 2 and n_solves >= T
    print(f"{tag}: max deviation from the oracle {worst:.2e} (tolerance {tol:.0e})")


# ---- 4. storage and launch splitting -------------------------------------------------------------------------------------------------
def test_f32_storage_follows_the_f64_run():
    nc, T = 10, 40
    ref = S.fleet_split_oracle(nc)
    a = fleet_controller(nc, "f64", stand_in=False, round32=True)
    b = fleet_controller(nc, "f32", stand_in=False, round32=True)
    assert b.X.dtype == torch.float32 and b.yaw.dtype == torch.float32 and b.seen.dtype == torch.int64
    _, aX, _, _, aS = a.control_step(T, record=True)
    _, bX, _, _, bS = b.control_step(T, record=True)
    assert b.obs_sel.dtype == torch.float32 and b.u_ref.dtype == torch.float32 and b.track.dtype == torch.int32
    aX, bX, aS, bS = cpu(aX), cpu(bX).astype(np.float64), u64(aS), u64(bS)
    dev = np.abs(aX - bX).max(axis=(0, 2))
    clear = np.array([float(r["min_margin"]) > 1e-3 for r in ref])                # over the oracle's 120 steps: no fewer than these 40
    print(f"f32 against f64 over {T} steps: max |X| difference {dev.max():.2e} (agent {int(dev.argmax())}); "
          f"{int(clear.sum())} agents with sighting margins above 1e-3; frozen in f64 / f32: {int((cpu(a.ret) != 0).sum())} / {int((cpu(b.ret) != 0).sum())}")
    assert clear.sum() > 20
    assert dev.max() < 1e-4
    assert np.array_equal(aS[:, clear], bS[:, clear]) and (aS[-1, clear] != 0).any()


def test_two_launches_equal_one():
    sc = S.FEATURE_SCENES["di"]
    out = []
    for split in ([30], [15, 15]):
        ctl = feature_controller(sc)
        for k in split:
            ctl.control_step(k)
        assert ctl.steps_done == 30
        out.append({name: cpu(getattr(ctl, name)) for name in ("X", "yaw", "u_att", "seen", "ret", "ret_step", "state_machine", "u_pos",
                                                                "u_prev", "obs_sel", "u_ref", "track", "current_goal_index")})
    for name, a in out[0].items():
        assert same_bits(a, out[1][name]), name                                  # bits: NaN positions of u_att included
    assert (out[0]["seen"] != 0).any() and np.isnan(out[0]["u_att"]).sum() < 3
