"""GPU: the fused arm rollout (csrc/manip_cbf_qp.hip: manip_rollout_kernel<1..4>) through BatchedManipulatorTracking against
oracle.manipulator.ArmTrackingOracle, 24 arms, on the scenes of tests/_manip_rollout_cases.py: every instantiation of the kernel,
a row cap that ends inside an obstacle, cbf_alpha off 1, a base inside an obstacle, launch splits, f32 storage, position in the
batch.  Trajectories and inputs at 1e-7 on every step (the figure of tests/test_manipulator_gpu.py); return codes, return steps,
state machine, goal index and goal equal.

Link geometry cannot be varied here: BatchedManipulatorTracking takes no link_lengths and always passes the reference's
(80, 70, 50)/60.  manip_qp, which the rollout shares with the single-solve kernel, is held to other link lengths in
tests/test_manip_qp_cases_gpu.py.

What the oracle gives on the scenes (asserted below; arm-steps on which the barrier changed the nominal input, return codes):
  m1        RPL 1   1492 changed   18 reached, 6 running
  m6        RPL 3   2393 changed   3 at -2, 5 reached, 16 running
  m10       RPL 4   1317 changed   13 at -2, 11 running
  m10cap60  RPL 2   2560 changed   6 reached, 18 running
  m5rows3   RPL 1   859 changed    19 reached, 5 running
18 of the 24 arms start in 'stop' (first waypoint outside the field of view)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _manip_rollout_cases as R  # noqa: E402
import safe_control_amd as sca  # noqa: E402

SPEC = dict(R.SPEC, model="Manipulator2D")
STATE = ("X", "u_pos", "ret", "ret_step", "state_machine", "current_goal_index", "goal")


def controller(q0, wl, obs, nc, io="f64", **spec):
    ctl = sca.BatchedManipulatorTracking(q0, dict(SPEC, num_constraints=nc, **spec), base_pos=R.BASE, obs=obs, io_dtype=io)
    ctl.set_waypoints(wl)
    return ctl


def rollout(ctl, chunks):
    tX, tU = [], []
    for n in chunks:
        _, x, u = ctl.control_step(n, record=True)
        tX.append(x.double().cpu().numpy()); tU.append(u.double().cpu().numpy())
    torch.cuda.synchronize()
    return np.concatenate(tX), np.concatenate(tU)


def state(ctl):
    return {k: getattr(ctl, k).cpu().numpy().copy() for k in STATE}


def hold_to_oracle(tag, ctl, tX, tU, o, atol=1e-7, excused=()):
    st = state(ctl)
    ok = np.array([i not in excused for i in range(len(o["ret"]))])
    dX, dU = float(np.abs(tX - o["X"])[:, ok].max()), float(np.abs(tU - o["U"])[:, ok].max())
    print(f"{tag}: max|X - X_oracle| = {dX:.3g}, max|U - U_oracle| = {dU:.3g}, ret {np.unique(st['ret'], return_counts=True)}")
    assert dX <= atol and dU <= atol
    assert np.array_equal(st["ret"][ok], o["ret"][ok]) and np.array_equal(st["ret_step"][ok], o["ret_step"][ok])
    assert np.array_equal(st["state_machine"][ok], o["sm"][ok]) and np.array_equal(st["current_goal_index"][ok], o["wp"][ok])
    assert np.array_equal(st["goal"][ok, 2], o["goal"][ok, 2])
    v = ok & (o["goal"][:, 2] != 0)
    np.testing.assert_allclose(st["goal"][v, :2], o["goal"][v, :2], rtol=0, atol=atol)
    np.testing.assert_allclose(st["X"][ok], o["X"][-1][ok], rtol=0, atol=atol)
    np.testing.assert_allclose(st["u_pos"][ok], o["U"][-1][ok], rtol=0, atol=atol)


@pytest.mark.parametrize("name", list(R.SCENES))
def test_every_instantiation_matches_the_oracle(name):
    """One launch of T steps per scene; the scene's (M, num_constraints) selects manip_rollout_kernel<RPL> (module docstring)."""
    s = R.scene(name)
    o = s["oracle"]
    assert R.rpl_of(len(s["obs"]), s["nc"]) == s["rpl"]
    assert o["n_changed"] > 20 and len(set(np.unique(o["ret"])) & {0, -1, -2}) >= 2 and o["stop0"] == 18
    ctl = controller(s["q0"], s["wl"], s["obs"], s["nc"])
    tX, tU = rollout(ctl, [s["T"]])
    hold_to_oracle(name, ctl, tX, tU, o)


@pytest.mark.parametrize("alpha", [0.3, 4.0])
def test_cbf_alpha_off_its_default(alpha):
    s = R.scene("m6", alpha=alpha, steps=60)
    assert s["oracle"]["n_changed"] > 20
    base = R.scene("m6")["oracle"]
    assert np.abs(s["oracle"]["X"] - base["X"][:60]).max() > 1e-3          # alpha matters on this scene
    ctl = controller(s["q0"], s["wl"], s["obs"], s["nc"], cbf_alpha=alpha)
    tX, tU = rollout(ctl, [60])
    hold_to_oracle(f"m6 alpha={alpha}", ctl, tX, tU, s["oracle"])


@pytest.mark.parametrize("case", ["in_the_qp_too", "collision_test_alone"])
def test_base_inside_an_obstacle(case):
    """Every arm ends -2 at step 0 and never moves.  'in_the_qp_too': the obstacle is the nearest one, so its base-circle row
    0.u + h >= 0 with h < 0 makes the QP infeasible as well.  'collision_test_alone': num_constraints = 1 hands the QP only a
    small nearer obstacle; the large one behind it contains the base and only the collision test sees it."""
    q0, wl = R.arms()
    T = 6
    if case == "in_the_qp_too":
        obs, nc = np.array([[R.BASE[0] + 0.2, R.BASE[1] + 0.1, 0.3, 0, 0, 0, 0], [R.BASE[0] + 2.5, R.BASE[1], 0.3, 0, 0, 0, 0]]), 150
    else:
        obs, nc = np.array([[R.BASE[0] - 1.0, R.BASE[1], 0.9, 0, 0, 0, 0], [R.BASE[0], R.BASE[1] + 0.7, 0.1, 0, 0, 0, 0]]), 1
    o = R.oracle_run(q0, wl, obs, nc, T)
    assert np.all(o["ret"] == -2) and np.all(o["ret_step"] == 0) and np.all(o["X"] == q0[None])
    ctl = controller(q0, wl, obs, nc)
    tX, tU = rollout(ctl, [T])
    assert np.array_equal(tX, np.broadcast_to(q0, (T, R.B, 3))) and np.all(tU == 0)
    hold_to_oracle(case, ctl, tX, tU, o)


def test_launch_split_does_not_change_a_bit():
    s = R.scene("m6")
    T = s["T"]
    runs = []
    for chunks in ([1] * T, [T], [7, 64, T - 71]):
        ctl = controller(s["q0"], s["wl"], s["obs"], s["nc"])
        tX, tU = rollout(ctl, chunks)
        runs.append((tX, tU, state(ctl)))
    for tX, tU, st in runs[1:]:
        assert np.array_equal(tX, runs[0][0]) and np.array_equal(tU, runs[0][1])
        for k in STATE:
            assert np.array_equal(st[k], runs[0][2][k]), k


def test_f32_storage_first_steps():
    """f32 arrays, arithmetic still f64: 30 steps against the oracle started from the states, waypoints, goals and table READ BACK
    from the controller (so both sides see the same rounded inputs), at 3e-6, the figure of the other fused loops.  Return codes
    equal, except for arms with a reached / rotate / feasibility decision of the oracle within 1e-5 of its threshold: at most
    2 % of the arms (none of 24; on the CPU the oracle's closest decision on this scene is printed below)."""
    s = R.scene("m6")
    T = 30
    ctl = controller(s["q0"], s["wl"], s["obs"], s["nc"], io="f32")
    q0 = ctl.X.double().cpu().numpy()
    wps, n_wp = ctl.waypoints.double().cpu().numpy(), ctl.n_wp.cpu().numpy()
    idx, sm, goal = ctl.current_goal_index.cpu().numpy(), ctl.state_machine.cpu().numpy(), ctl.goal.double().cpu().numpy()
    names = {v: k for k, v in R.SM.items()}
    start = [dict(waypoints=wps[i, : n_wp[i]], index=idx[i], sm=names[int(sm[i])], goal=goal[i, :2] if goal[i, 2] != 0 else None)
             for i in range(R.B)]
    o = R.oracle_run(q0, None, ctl.obs.double().cpu().numpy(), s["nc"], T, start=start, watch=True)
    print("closest decision per arm:", np.sort(o["near"])[:4])
    excused = [i for i in range(R.B) if o["near"][i] < 1e-5]
    assert len(excused) <= R.B * 2 // 100
    assert o["n_changed"] > 20
    tX, tU = rollout(ctl, [T])
    hold_to_oracle("m6 f32", ctl, tX, tU, o, atol=3e-6, excused=excused)


def test_position_in_the_batch_does_not_matter():
    """Thirty copies of the 24 arms in one launch (B = 720) stay bit-identical to one another, and arm 0 equals a B = 1 run."""
    s = R.scene("m6")
    T, n = s["T"], 30
    ctl = controller(np.tile(s["q0"], (n, 1)), list(s["wl"]) * n, s["obs"], s["nc"])
    tX, tU = rollout(ctl, [T])
    st = state(ctl)
    tX, tU = tX.reshape(T, n, R.B, 3), tU.reshape(T, n, R.B, 3)
    assert np.array_equal(tX, np.broadcast_to(tX[:, :1], tX.shape)) and np.array_equal(tU, np.broadcast_to(tU[:, :1], tU.shape))
    for k in STATE:
        a = st[k].reshape((n, R.B) + st[k].shape[1:])
        assert np.array_equal(a, np.broadcast_to(a[:1], a.shape)), k
    np.testing.assert_allclose(tX[:, 0], s["oracle"]["X"], rtol=0, atol=1e-7)
    one = controller(s["q0"][:1], s["wl"][:1], s["obs"], s["nc"])
    oX, oU = rollout(one, [T])
    assert np.array_equal(oX[:, 0], tX[:, 0, 0]) and np.array_equal(oU[:, 0], tU[:, 0, 0])
    so = state(one)
    for k in STATE:
        assert np.array_equal(so[k][0], st[k][0]), k
