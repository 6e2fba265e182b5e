"""GPU: the sensing rollout (csrc/tracking_sense.hip, BatchedSensingTrackingController) against the reference's own runs
(tests/golden/unknown_env.npz) and the float64 oracle (tests/_unknown_env_oracle.py): unknown obstacles sighted through the camera
cone, their memory, their collisions, and the integrators' yaw under the 'simple' and 'velocity_tracking_yaw' attitude controllers.

Tolerances are the ones tests/test_tracking_gpu.py holds these models to over whole closed loops: 1e-7 for the integrators, 1e-6 for
the unicycle.  Events (state machine, return codes, the step they happen at, the mask of sighted rows) must be equal; the fixture's
and the fleet's sightings are decided by margins far above those tolerances (the generator and tests/test_oracle_unknown_env.py
check that)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import safe_control_amd as sca  # noqa: E402
import _unknown_env_oracle as O  # noqa: E402
from oracle import robots as R  # noqa: E402

pytestmark = pytest.mark.gpu

ALL_SEEN = np.uint64(2 ** 64 - 1)


def cpu(t):
    return t.detach().cpu().numpy()


def u64(t):
    return cpu(t).view(np.uint64)


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "unknown_env.npz"))


def controller_from_fixture(z, tag, X0=None, io_dtype="f64"):
    mi = int(z[f"{tag}/model"])
    spec = dict(O.fixture_spec(z, tag), model=O.MODEL_NAMES[mi])
    ctype = {"pos": "cbf_qp"}
    if O.ATTS[int(z[f"{tag}/att"])] is not None:
        ctype["att"] = O.ATTS[int(z[f"{tag}/att"])]
    ctl = sca.BatchedSensingTrackingController(z[f"{tag}/x0"][None, :] if X0 is None else X0, spec, controller_type=ctype,
                                               obs=z[f"{tag}/obs"], unknown_obs=z[f"{tag}/unknown"], io_dtype=io_dtype)
    ctl.set_waypoints(z[f"{tag}/waypoints"])
    return ctl


# ---- 1. the five reference runs, one agent each ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", O.FIXTURE_TAGS)
def test_reference_runs(fixture, tag):
    z = fixture
    n = len(z[f"{tag}/ret"])
    ctl = controller_from_fixture(z, tag)
    tol = 1e-6 if int(z[f"{tag}/model"]) == 0 else 1e-7
    assert int(ctl.state_machine[0]) == int(z[f"{tag}/sm0"])
    tX, tU, tY, tS = [], [], [], []
    done = 0
    for k in (1, 199, n - 200 + 5):                                          # the last launch runs 5 steps past the reference's end
        ret, a, b, c, d = ctl.control_step(k, record=True)
        tX.append(cpu(a)[:, 0]); tU.append(cpu(b)[:, 0]); tY.append(cpu(c)[:, 0]); tS.append(u64(d)[:, 0])
        done += k
        if done <= n or int(z[f"{tag}/ret"][-1]) != 0:                         # (a frozen agent keeps its state; a running one moves on)
            assert int(ctl.state_machine[0]) == int(z[f"{tag}/sm"][min(done, n) - 1]), f"state machine after {done} steps"
    tX, tU, tY, tS = np.concatenate(tX), np.concatenate(tU), np.concatenate(tY), np.concatenate(tS)
    nx = z[f"{tag}/X"].shape[1]
    print(f"{tag}: max |X - ref| {np.abs(tX[:n, :nx] - z[f'{tag}/X']).max():.2e}, |U - ref| {np.abs(tU[:n] - z[f'{tag}/U']).max():.2e}, "
          f"|yaw - ref| {np.abs(tY[:n] - z[f'{tag}/yaw']).max():.2e}")
    np.testing.assert_allclose(tX[:n, :nx], z[f"{tag}/X"], rtol=tol, atol=tol)
    np.testing.assert_allclose(tU[:n], z[f"{tag}/U"], rtol=tol, atol=tol)
    np.testing.assert_allclose(tY[:n], z[f"{tag}/yaw"], rtol=tol, atol=tol)
    assert np.array_equal(tS[:n], z[f"{tag}/mask"])
    last = int(z[f"{tag}/ret"][-1])
    assert int(ctl.ret[0]) == last and int(ctl.ret_step[0]) == (n - 1 if last != 0 else -1)
    assert int(ctl.current_goal_index[0]) == int(z[f"{tag}/idx"][-1]) or last == 0
    if last != 0:                                                            # a frozen agent repeats its last row
        for arr in (tX, tU, tY, tS):
            assert all(np.array_equal(arr[n - 1], arr[j]) for j in range(n, n + 5))
        ua_ref = z[f"{tag}/u_att"][-1]
        if last == -1 and not np.isnan(ua_ref):
            np.testing.assert_allclose(float(ctl.u_att[0]), ua_ref, rtol=tol, atol=tol)


# ---- 2. a batch against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_constraints", [10, 5])                        # KMAX 16 and 8
def test_batch_against_the_oracle(num_constraints):
    sc = O.fleet_scene()
    ref = O.fleet_oracle(num_constraints)
    spec = dict(O.FLEET_SPEC, model="DoubleIntegrator2D", num_constraints=num_constraints)
    ctl = sca.BatchedSensingTrackingController(sc["X0"], spec, obs=sc["obs"], unknown_obs=sc["unknown"])
    ctl.set_waypoints(sc["waypoints"])
    assert ctl.B == 130 and ctl.unknown_obs.shape[0] == 33 and ctl.obs.shape[0] == 12
    ret, tX, tU, tY, tS = ctl.control_step(O.FLEET_STEPS, record=True)
    tX, tU, tY, tS, ret, rstep, sm = cpu(tX), cpu(tU), cpu(tY), u64(tS), cpu(ret), cpu(ctl.ret_step), cpu(ctl.state_machine)
    excluded, worst = [], 0.0
    for i, r in enumerate(ref):
        if float(r["min_margin"]) < 1e-6:                                    # a sighting decided by less than the comparison's tolerance
            excluded.append(i)
            continue
        n = len(r["ret"])
        worst = max(worst, np.abs(tX[:n, i] - r["X"]).max(), np.abs(tU[:n, i] - r["U"]).max(), np.abs(tY[:n, i] - r["yaw"]).max())
        np.testing.assert_allclose(tX[:n, i], r["X"], rtol=1e-7, atol=1e-7, err_msg=f"agent {i}")
        np.testing.assert_allclose(tU[:n, i], r["U"], rtol=1e-7, atol=1e-7, err_msg=f"agent {i}")
        np.testing.assert_allclose(tY[:n, i], r["yaw"], rtol=1e-7, atol=1e-7, err_msg=f"agent {i}")
        assert np.array_equal(tS[:n, i], r["mask"]), f"agent {i}: sighted rows"
        last = int(r["ret"][-1])
        assert ret[i] == last and rstep[i] == (n - 1 if last != 0 else -1) and sm[i] == r["sm"][-1], f"agent {i}"
    print(f"num_constraints {num_constraints}: excluded {excluded}, max deviation from the oracle {worst:.2e}")
    assert len(excluded) <= 2


@pytest.mark.parametrize("io", ["f64", "f32"])
@pytest.mark.parametrize("big", [False, True], ids=["m3", "m1171"])
@pytest.mark.parametrize("num_constraints", [8, 9])                         # KMAX 8 and 16
@pytest.mark.parametrize("name", sca.BatchedSensingTrackingController.MODELS)
def test_every_kernel_of_the_sensing_launcher(name, num_constraints, big, io):
    """tracking_sense_kernel for its three models, KMAX 8 and 16 and both storage types: 65 agents x 10 steps on three known and five
    unknown circles, and 3 agents x 2 steps on a known table of 1171 rows (65 576 B of LDS: the raised dynamic-LDS limit), one launch
    against the oracle.  f64: 1e-7, the figure of the test above.  f32: the inputs are f32 numbers and the state stays in f64
    registers for the whole launch, so the records differ by their rounding to f32 alone, 2^-24 relative: 1e-7 + 2^-24."""
    import _agent_params_cases as AC
    T = AC.BIG_T if big else AC.RUNG_T
    case = AC.rung_case(name, False, big)
    ctl = sca.BatchedSensingTrackingController(case["X0"], dict(case["specs"][0], num_constraints=num_constraints), obs=case["obs"],
                                               unknown_obs=O.RUNG_UNKNOWN, io_dtype=io)
    ctl.set_waypoints(case["wl"])
    ret, tX, tU, tY, tS = ctl.control_step(T, record=True)
    ref = O.rung_records(case, T, num_constraints)
    O.assert_records(ref, cpu(tX.double()), cpu(tU.double()), cpu(tY.double()), u64(tS), cpu(ret), cpu(ctl.ret_step), cpu(ctl.state_machine),
                     1e-7 + (2.0 ** -24 if io == "f32" else 0.0))
    if not big:
        assert any(r["mask"].any() for r in ref)                             # some agent sighted an unknown row


# ---- 3. the edges of Mu -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["DynamicUnicycle2D", "DoubleIntegrator2D"])
def test_no_unknown_rows_is_the_plain_rollout_bit_for_bit(golden_dir, monkeypatch, model):
    """Mu = 0: the same arithmetic as tracking_rollout_kernel, hence the same bits."""
    rng = np.random.default_rng(11)
    B, T = 130, 300
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
    monkeypatch.setenv("SC_TRACK_LANE_PER_AGENT", "1")
    base = sca.BatchedTrackingController(X0, dict(spec), enable_rotation=rot, obs=obs)
    base.set_waypoints(wps)
    base.control_step(T)
    new = sca.BatchedSensingTrackingController(X0, dict(spec), enable_rotation=rot, obs=obs, unknown_obs=None)
    new.set_waypoints(wps)
    new.control_step(T)
    assert new.unknown_obs.shape[0] == 0
    for name in ("X", "u_pos", "ret", "ret_step", "state_machine"):
        a, b = cpu(getattr(base, name)), cpu(getattr(new, name))
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    assert int(new.seen.abs().sum()) == 0
    moved = np.linalg.norm(cpu(new.X)[:, :2] - X0[:, :2], axis=1)
    assert (moved > 1.0).sum() > B // 2 and (cpu(new.state_machine) == 1).any()      # the run is not a trivial one


def test_one_unknown_row(fixture):
    z = fixture
    rng = np.random.default_rng(5)
    B, T = 3, 160
    X0 = np.tile(z["di_vty/x0"], (B, 1))
    X0[:, :2] += rng.uniform(-0.2, 0.2, (B, 2))
    X0[:, 4] = [1.2, 1.9, 0.4]
    unknown = np.array([[2.4, 5.0, 0.4]])
    ctl = sca.BatchedSensingTrackingController(X0, {"model": "DoubleIntegrator2D", "radius": 0.25, "v_max": 1.0, "a_max": 1.0},
                                               obs=z["di_vty/obs"], unknown_obs=unknown)
    ctl.set_waypoints(z["di_vty/waypoints"])
    ret, tX, tU, tY, tS = ctl.control_step(T, record=True)
    tX, tU, tY, tS = cpu(tX), cpu(tU), cpu(tY), u64(tS)
    sightings = 0
    for i in range(B):
        o = O.UnknownEnvOracle(R.MODEL_DI, X0[i, :4], O.FLEET_SPEC, obs=z["di_vty/obs"], unknown_obs=unknown, yaw0=X0[i, 4])
        o.set_waypoints(z["di_vty/waypoints"])
        r = O.run(o, T)
        n = len(r["ret"])
        assert o.min_margin > 1e-6
        np.testing.assert_allclose(tX[:n, i], r["X"], rtol=1e-7, atol=1e-7)
        np.testing.assert_allclose(tU[:n, i], r["U"], rtol=1e-7, atol=1e-7)
        np.testing.assert_allclose(tY[:n, i], r["yaw"], rtol=1e-7, atol=1e-7)
        assert np.array_equal(tS[:n, i], r["mask"]) and int(ctl.ret[i]) == int(r["ret"][-1])
        sightings += int(r["mask"][-1])
    assert sightings > 0


def test_sixty_four_unknown_rows_all_in_the_cone():
    ang = np.deg2rad(np.linspace(-30.0, 30.0, 8))
    rad = np.linspace(1.0, 2.75, 8)
    unknown = np.array([[r * np.cos(a), r * np.sin(a), 0.05] for r in rad for a in ang])
    assert unknown.shape == (64, 3)
    X0 = np.array([[0.0, 0.0, 0.3, 0.0, 0.0]])
    spec = {"radius": 0.25, "v_max": 1.0, "a_max": 1.0, "num_constraints": 16}
    wps = np.array([[0.0, 0.0], [10.0, 0.0]])
    ctl = sca.BatchedSensingTrackingController(X0, dict(spec, model="DoubleIntegrator2D"), unknown_obs=unknown)
    ctl.set_waypoints(wps)
    assert int(ctl.state_machine[0]) == 1                                    # the goal is in view: 'track'
    ret, tX, tU, tY, tS = ctl.control_step(1, record=True)
    assert u64(ctl.seen)[0] == ALL_SEEN and u64(tS)[0, 0] == ALL_SEEN
    o = O.UnknownEnvOracle(R.MODEL_DI, X0[0, :4], spec, unknown_obs=unknown, num_constraints=16, yaw0=0.0)
    o.set_waypoints(wps)
    r = O.run(o, 1)
    assert o.min_margin > 1e-6 and int(r["mask"][0]) == 2 ** 64 - 1
    assert int(ret[0]) == int(r["ret"][0])
    np.testing.assert_allclose(cpu(tX)[0, 0], r["X"][0], rtol=1e-7, atol=1e-7)
    np.testing.assert_allclose(cpu(tU)[0, 0], r["U"][0], rtol=1e-7, atol=1e-7)
    np.testing.assert_allclose(cpu(tY)[0, 0], r["yaw"][0], rtol=1e-7, atol=1e-7)
    np.testing.assert_allclose(float(ctl.u_att[0]), r["u_att"][0], rtol=1e-7, atol=1e-7)


# ---- 4. how a run is cut into launches does not matter ----------------------------------------------------------------------------
def test_launch_split_gives_identical_bits(fixture):
    z = fixture
    rng = np.random.default_rng(3)
    B = 70
    X0 = np.tile(z["di_se/x0"], (B, 1))
    X0[:, :2] += rng.uniform(-0.4, 0.4, (B, 2))
    X0[:, 2:4] = rng.uniform(-0.2, 0.2, (B, 2))
    X0[:, 4] = rng.uniform(-np.pi, np.pi, B)
    out = []
    for split in ([1] * 300, [300], [7, 64, 229]):
        ctl = controller_from_fixture(z, "di_se", X0=X0)
        for k in split:
            ctl.control_step(k)
        assert ctl.steps_done == 300
        out.append({name: cpu(getattr(ctl, name)) for name in ("X", "yaw", "u_att", "seen", "ret", "ret_step", "state_machine", "u_pos")})
    for other in out[1:]:
        for name, a in out[0].items():
            assert np.array_equal(a.view(np.uint8), other[name].view(np.uint8)), name      # bits: NaN positions of u_att included
    assert (out[0]["seen"] != 0).any() and np.isnan(out[0]["u_att"]).sum() < B


# ---- 5. f32 storage ---------------------------------------------------------------------------------------------------------------
def test_f32_storage_rounds_the_f64_step(fixture):
    z = fixture
    rng = np.random.default_rng(9)
    B = 70
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)         # inputs both storages hold exactly
    X0 = np.zeros((B, 5))
    X0[:, 0] = 2.0 + rng.uniform(-0.4, 0.4, B)
    X0[:, 1] = rng.uniform(2.0, 7.0, B)
    X0[:, 2:4] = rng.uniform(-0.5, 0.5, (B, 2))
    X0[:, 4] = np.pi / 2 + rng.uniform(-0.5, 0.5, B)                         # most look at the waypoint ahead: 'track'
    X0 = f32(X0)
    unknown = f32(z["di_se/unknown"])
    spec = {"model": "DoubleIntegrator2D", "radius": 0.25, "v_max": 1.0, "a_max": 1.0}
    res = {}
    for io in ("f64", "f32"):
        ctl = sca.BatchedSensingTrackingController(X0, dict(spec), obs=f32(z["di_se/obs"]), unknown_obs=unknown, io_dtype=io)
        ctl.set_waypoints(f32(np.array([[2.0, 12.0], [12.0, 12.0]])))
        ctl.control_step(1)
        res[io] = ctl
    a, b = res["f64"], res["f32"]
    assert b.X.dtype == torch.float32 and b.yaw.dtype == torch.float32 and b.seen.dtype == torch.int64
    assert (cpu(a.state_machine) == 1).sum() > B // 2 and np.array_equal(cpu(a.state_machine), cpu(b.state_machine))
    for name in ("X", "yaw", "u_pos"):
        want = cpu(getattr(a, name)).astype(np.float32)
        assert np.array_equal(want.view(np.uint32), cpu(getattr(b, name)).view(np.uint32)), name
    assert np.array_equal(cpu(a.seen), cpu(b.seen)) and (cpu(a.seen) != 0).any()
    assert np.array_equal(cpu(a.ret), cpu(b.ret))
