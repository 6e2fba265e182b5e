"""GPU tests of the fused closed loop under 'optimal_decay_cbf_qp' (csrc/tracking_od.hip) against tests/_od_tracking_oracle.py, the
float64 restatement of the reference's control_step with that controller (checked on the CPU by tests/test_oracle_od_tracking.py)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import _od_tracking_oracle as O  # noqa: E402
import safe_control_amd as sca  # noqa: E402
from safe_control_amd import _lib  # noqa: E402

DEV = "cuda:0"
OD = {"pos": "optimal_decay_cbf_qp"}
B, T, LAUNCHES = 136, 100, (37, 63)          # two full blocks and a ragged tail of 8; state, ret_step, omega, min_h cross a launch boundary
TIE = 1e-7                                   # an agent may be left out only if the ORACLE's selection came this close to a tie
P1 = dict(p_sb1=1.0, p_sb2=1.0)              # small penalties: the decay moves (with the default 1e4 it stays within 1e-4 of 1)

# name: (model, robot_spec additions, optimal-decay parameter overrides, enable_rotation, dyn_obs, seed)
RUNS = {
    "du": ("DynamicUnicycle2D", {}, P1, False, False, 0),
    "du_default_penalty": ("DynamicUnicycle2D", {}, {}, False, False, 0),
    "du_rotate": ("DynamicUnicycle2D", {"exploration": True}, P1, True, False, 0),
    "kb": ("KinematicBicycle2D", {}, P1, False, False, 0),
    "c3bf_moving": ("KinematicBicycle2D_C3BF", {}, dict(p_sb1=1.0), False, True, 0),
    "dpcbf_moving": ("KinematicBicycle2D_DPCBF", {}, dict(p_sb1=1.0), False, True, 17),
}
# The seeds were chosen on the CPU, from the oracle alone, by two counts that every parity test asserts again: no agent within TIE of a
# selection tie, and no step on which oracle/od_cbf_qp.py reports 'infeasible' for a QP that has a solution by construction (an
# obstacle with h != 0: the decay variable alone satisfies the row).  The second used to happen to the DPCBF bicycle when the row and
# both input bounds are active: its steering coefficient is ~1e2, and the oracle's determinant test, then scaled by |K|max^3, skipped
# that nearly singular active set and found no other; seeds 0 .. 30 of this generator had 0 .. 11 such steps among 136 agents x 100
# steps, and 5, 7, 13 and 17 had none.  The oracle now eliminates the inputs held at a bound and tests singularity free of scale
# (tests/test_oracle_od_tracking.py pins one such QP, tests/test_od_qp_cases.py holds it to a certificate on that whole class), so the
# count can only have fallen and stays asserted as a guard.  Seed 17 is kept: it has the most agents ending in -2 (42, all collisions).


def setup(name, io="f64", B_=B):
    model, extra, odp, rot, dyn, seed = RUNS[name]
    X0, wps, obs = O.scene(model, B_, seed, moving=dyn)
    base = dict(O.DU_SPEC if model == "DynamicUnicycle2D" else O.KB_SPEC, model=model, **extra)
    cfg = dict(model=model, spec=base, od_param=odp, dt=0.05, dyn_obs=dyn, enable_rotation=rot)
    spec = dict(base, **{"cbf_" + k: v for k, v in odp.items()})
    ctl = sca.BatchedTrackingController(X0, spec, controller_type=OD, dt=0.05, enable_rotation=rot, obs=obs, dyn_obs=dyn, io_dtype=io)
    ctl.set_waypoints(list(wps))
    return ctl, cfg, X0, wps, obs


def rollout(ctl, launches):
    out = [[], [], []]
    for n in launches:
        ret, tX, tU, tW = ctl.control_step(n, record=True)
        for o, t in zip(out, (tX, tU, tW)):
            o.append(t.double().cpu().numpy())
    return [np.concatenate(o) for o in out]


def compare(ctl, traj, r, tol, steps, full):
    """Trajectories up to each kept agent's last oracle step; with `full` also the final ret / ret_step / min_h / state machine."""
    tX, tU, tW = traj
    keep = r["min_margin"] >= TIE
    assert (~keep).mean() <= 0.02, f"{int((~keep).sum())} agents within {TIE} of a selection tie"
    assert int(r["rejected_feasible"].sum()) == 0, "the oracle left its range of validity on this scene (see RUNS)"
    n = np.minimum(r["n"], steps)
    valid = (np.arange(steps)[None, :] < n[:, None]) & keep[:, None]                    # [B, steps]
    for name, got, want in (("X", tX, r["X"]), ("U", tU, r["U"]), ("omega", tW, r["W"])):
        got = np.swapaxes(got, 0, 1)[:, :steps]
        used = np.abs(got - want[:, :steps])[valid] / (tol + tol * np.abs(want[:, :steps][valid]))
        print(f"{name}: max |gpu - oracle| / (atol + rtol |oracle|) over {int(valid.sum())} agent-steps = {used.max():.3e}")
        np.testing.assert_allclose(got[valid], want[:, :steps][valid], rtol=tol, atol=tol, err_msg=name)
    if not full:
        return keep
    ret, rstep = ctl.ret.cpu().numpy(), ctl.ret_step.cpu().numpy()
    k = np.flatnonzero(keep)
    assert np.array_equal(ret[k], r["ret"][k])
    done = k[r["ret"][k] != 0]
    assert np.array_equal(rstep[done], r["n"][done] - 1)
    assert (rstep[k[r["ret"][k] == 0]] == -1).all()
    np.testing.assert_allclose(ctl.min_h.double().cpu().numpy()[k], r["min_h"][k], rtol=tol, atol=tol)
    np.testing.assert_allclose(ctl.omega.double().cpu().numpy()[k], r["W"][k, r["n"][k] - 1], rtol=tol, atol=tol)
    assert np.array_equal(ctl.state_machine.cpu().numpy()[k], r["sm_final"][k])
    assert np.array_equal(ctl.current_goal_index.cpu().numpy()[k], r["wp_final"][k])
    return keep


@pytest.mark.parametrize("name", list(RUNS))
def test_oracle_parity_f64(name):
    """100 steps in launches of 37 + 63 against the oracle at rtol = atol = 1e-6, the figure every fused-loop test of
    tests/test_tracking_gpu.py uses against oracle/tracking.py."""
    ctl, cfg, X0, wps, obs = setup(name)
    traj = rollout(ctl, LAUNCHES)
    r = O.run_many(cfg, X0, wps, obs, T)
    keep = compare(ctl, traj, r, 1e-6, T, full=True)
    # the run is not vacuous: finished, failed, started in 'stop' (or in 'rotate' under exploration), and the decay moved
    moved = np.nanmax(np.abs(r["W"] - 1.0), axis=(1, 2))
    assert (r["ret"][keep] == -1).any() and (r["ret"][keep] == -2).any()
    if name == "du_rotate":
        assert (r["sm0"][keep] == O.SM_INDEX["rotate"]).any() and r["rotated"][keep].any()
    else:
        assert (r["sm0"][keep] == O.SM_INDEX["stop"]).any()
    if name == "du_default_penalty":
        assert 1e-7 < moved[keep].max() < 1e-3                   # p_sb = 1e4 pins the decay: it moves, by less than a part in a thousand
    else:
        assert (moved[keep] > 1e-3).any()
    if cfg["dyn_obs"]:
        want = obs.copy()
        for _ in range(T):
            want[:, 0:2] += want[:, 3:5] * 0.05
        np.testing.assert_allclose(ctl.obs.cpu().numpy(), want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ["du", "kb", "c3bf_moving", "dpcbf_moving"])
def test_oracle_parity_f32_storage_first_launch(name):
    """f32 storage, f64 arithmetic: the first launch against the oracle run from the states, waypoints and table re-read from the
    device, at 3e-6 as tests/test_odcbfqp_gpu.py does for single solves."""
    ctl, cfg, _, _, _ = setup(name, io="f32")
    X0 = ctl.X.double().cpu().numpy()
    obs = ctl.obs.double().cpu().numpy()
    nw = ctl.n_wp.cpu().numpy()
    assert (nw == 2).all()                                       # every route of the scene keeps both waypoints
    wps = ctl.waypoints.double().cpu().numpy()
    sm0 = ctl.state_machine.cpu().numpy().copy()
    traj = rollout(ctl, LAUNCHES[:1])
    r = O.run_many(cfg, X0, wps, obs, LAUNCHES[0])
    assert np.array_equal(sm0, r["sm0"])
    keep = compare(ctl, traj, r, 3e-6, LAUNCHES[0], full=False)
    assert keep.sum() >= 0.98 * B and (r["n"] < LAUNCHES[0]).any()


def big_table(obs):
    """The scene's rows, then small circles 500 m away up to 1171 rows: 65 576 B of LDS, the first table above the 64 KiB a kernel
    gets without the raised limit.  f32 numbers, so both storage types read the same table."""
    far = np.zeros((1171 - len(obs), 7))
    far[:, 0], far[:, 1], far[:, 2] = 500.0 + np.arange(len(far)), 500.0, 0.25
    return np.vstack([obs, far]).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("io,tol", [("f64", 1e-6), ("f32", 3e-6)])           # the figures of the two parity tests above
@pytest.mark.parametrize("name", ["du", "kb", "c3bf_moving", "dpcbf_moving"])
def test_table_above_64_kib_of_lds(name, io, tol):
    """M = 1171 rows, 3 agents, 2 steps in one launch against the oracle: every model's kernel with the raised dynamic-LDS limit."""
    model, extra, odp, rot, dyn, seed = RUNS[name]
    X0, wps, obs = O.scene(model, B, seed, moving=dyn)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    X0, wps, obs = f32(X0[:3]), f32(wps[:3]), big_table(obs)
    base = dict(O.DU_SPEC if model == "DynamicUnicycle2D" else O.KB_SPEC, model=model, **extra)
    cfg = dict(model=model, spec=base, od_param=odp, dt=0.05, dyn_obs=dyn, enable_rotation=rot)
    ctl = sca.BatchedTrackingController(X0, dict(base, **{"cbf_" + k: v for k, v in odp.items()}), controller_type=OD, dt=0.05,
                                        enable_rotation=rot, obs=obs, dyn_obs=dyn, io_dtype=io)
    ctl.set_waypoints(list(wps))
    assert ctl.obs.shape[0] * 56 > 64 * 1024
    traj = rollout(ctl, (2,))
    r = O._run_slice(cfg, X0, wps, obs, 2)
    keep = compare(ctl, traj, r, tol, 2, full=(io == "f64"))
    assert keep.all()


def test_no_obstacles_still_clips_to_the_input_box():
    """obs None: the optimal-decay QP is solved with a zero row, so the applied turn rate is clipped to w_max, where the same scene
    under 'cbf_qp' passes u_ref through unclipped (csrc/tracking.hip, M == 0)."""
    spec = dict(O.DU_SPEC)
    X0 = np.array([[0.0, 0.0, 0.0, 0.2]])
    wps = np.array([[2.0, 1.2], [2.0, 3.0]])
    err = np.arctan2(1.2, 2.0)
    assert 3.0 * err > spec["w_max"] and 2.0 * err > spec["w_max"]
    od = sca.BatchedTrackingController(X0, dict(spec), controller_type=OD, enable_rotation=False, obs=None)
    od.set_waypoints(wps)
    _, _, tU, tW = od.control_step(1, record=True)
    u = tU.cpu().numpy()[0, 0]
    assert u[1] == pytest.approx(spec["w_max"], abs=1e-12) and u[0] == pytest.approx(0.5 * (min(0.5 * (np.hypot(2.0, 1.2) - 0.05) * np.cos(err), 1.0) - 0.2), abs=1e-12)
    assert np.array_equal(tW.cpu().numpy()[0, 0], [1.0, 1.0]) and float(od.min_h[0].item()) == np.inf
    o = O.make_oracle(dict(model="DynamicUnicycle2D", spec=spec), X0[0], wps, None)
    o.control_step()
    np.testing.assert_allclose(od.X.cpu().numpy()[0], o.X, rtol=0, atol=1e-12)
    qp = sca.BatchedTrackingController(X0, dict(spec), controller_type={"pos": "cbf_qp"}, enable_rotation=False, obs=None)
    qp.set_waypoints(wps)
    _, _, tU2 = qp.control_step(1, record=True)
    assert tU2.cpu().numpy()[0, 0, 1] == pytest.approx(2.0 * err, abs=1e-12)


def test_one_step_equals_select_then_single_solve():
    """For agents in 'track', the input of a one-step rollout is the composition of existing calls: sc_tracking_select_batch with
    num_constraints = 1 and gains 3 / 0.5 / 0.5, then BatchedOptimalDecayCBFQP.solve on the row and reference it returns."""
    ctl, cfg, X0, wps, obs = setup("du")
    lib = _lib.load()
    p = ctl._od_params(1).track
    p.num_constraints = 1
    assert (p.k_omega, p.k_a, p.k_v) == (3.0, 0.5, 0.5)
    t64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=DEV)
    obs_sel, goal2, u_ref, track = t64(B, 1, 7), t64(B, 2), t64(B, 2), torch.empty(B, dtype=torch.int32, device=DEV)
    wp_i, sm, goal = ctl.current_goal_index.clone(), ctl.state_machine.clone(), ctl.goal.clone()
    rc = lib.sc_tracking_select_batch(C.byref(p), B, len(obs), ctl.X.data_ptr(), ctl.waypoints.data_ptr(), ctl.n_wp.data_ptr(), wp_i.data_ptr(),
                                      sm.data_ptr(), goal.data_ptr(), ctl.obs.data_ptr(), ctl.ret.data_ptr(), obs_sel.data_ptr(),
                                      goal2.data_ptr(), u_ref.data_ptr(), track.data_ptr(), None)
    _lib.check(rc, "sc_tracking_select_batch")
    solver = sca.BatchedOptimalDecayCBFQP(dict(ctl.robot_spec), dt=0.05, io_dtype="f64", compute_dtype="f64", cbf_param=dict(ctl.cbf_param))
    u, w, st, h = solver.solve(ctl.X.clone(), u_ref, obs_sel[:, 0].contiguous())
    ret, tX, tU, tW = ctl.control_step(1, record=True)
    m = ((track != 0) & (ret == 0)).cpu().numpy()
    assert m.sum() >= B // 2
    np.testing.assert_allclose(tU.cpu().numpy()[0][m], u.cpu().numpy()[m], rtol=0, atol=1e-12)
    np.testing.assert_allclose(tW.cpu().numpy()[0][m], w.cpu().numpy()[m], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ctl.min_h.cpu().numpy()[m], h.cpu().numpy()[m], rtol=0, atol=1e-12)


def test_moving_table_every_block_sees_the_same_table():
    """4096 agents (64 blocks) over a moving table: every block reads the table as it was at launch and advances its own copy, so the
    30 copies of each of the scene's 136 agents, which sit in different blocks and lanes, stay identical, agent 0 matches a run on
    its own, and the table ends where n steps of obs += v dt put it."""
    name, n_big, launches = "c3bf_moving", 4096, (25, 35)
    model, extra, odp, rot, dyn, seed = RUNS[name]
    X0, wps, obs = O.scene(model, B, seed, moving=True)
    idx = np.arange(n_big) % B
    spec = dict(O.KB_SPEC, model=model, **{"cbf_" + k: v for k, v in odp.items()})
    big = sca.BatchedTrackingController(X0[idx], dict(spec), controller_type=OD, enable_rotation=False, obs=obs, dyn_obs=True)
    big.set_waypoints(list(wps[idx]))
    one = sca.BatchedTrackingController(X0[:1], dict(spec), controller_type=OD, enable_rotation=False, obs=obs, dyn_obs=True)
    one.set_waypoints(list(wps[:1]))
    for n in launches:
        big.control_step(n)
        one.control_step(n)
    for a in ("X", "omega", "min_h", "ret", "ret_step", "u_pos"):
        g, s = getattr(big, a).cpu().numpy(), getattr(one, a).cpu().numpy()
        assert np.array_equal(g[0], s[0]), a
        copies = g[: (n_big // B) * B].reshape((n_big // B, B) + g.shape[1:])
        assert np.array_equal(copies, np.broadcast_to(copies[:1], copies.shape)), a
    assert (big.ret.cpu().numpy() != 0).any() and (big.ret.cpu().numpy() == 0).any()
    want = obs.copy()
    for _ in range(sum(launches)):
        want[:, 0:2] += want[:, 3:5] * 0.05
    np.testing.assert_allclose(big.obs.cpu().numpy(), want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(one.obs.cpu().numpy(), want, rtol=0, atol=1e-12)
