"""GPU tests of the fused Quad2D closed loop under 'cbf_qp' and 'optimal_decay_cbf_qp' (csrc/tracking_quad_qp.hip) against
tests/_quad2d_qp_tracking_oracle.py, the float64 restatement of the reference's control_step for that robot and those controllers
(held on the CPU to the reference's own run by tests/test_oracle_quad2d_qp_tracking.py)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import _quad2d_qp_tracking_oracle as Q  # noqa: E402
import safe_control_amd as sca  # noqa: E402
from safe_control_amd import _lib  # noqa: E402

DEV = "cuda:0"
B, T, LAUNCHES = 136, 120, (37, 83)          # two full blocks and a tail of 8; state, ret_step, omega, min_h cross a launch boundary
TIE = 1e-7                                   # an agent may be left out only if the ORACLE's selection came this close to a tie
P1 = dict(p_sb1=1.0, p_sb2=1.0)              # small penalties: the decay moves

# name: (controller, num_constraints, optimal-decay parameter overrides, dyn_obs, seed).  K = 3 and 1 run the kernel built for up to 4
# rows, K = 6 the one for up to 8, K = 10 (the reference's default) the one for up to 16: every instantiation the launcher can pick.
# The seeds were chosen on the CPU, from the oracle alone, by the counts every parity test asserts again (Q.scene, seeds 0 .. 5, 120
# steps: no agent within 2e-6 of a selection tie, no optimal-decay step outside the oracle's range of validity; seed 0: 13 / 19 / 104
# agents end -1 / -2 / running under 'cbf_qp' with K = 3, 16 of the -2 on an infeasible QP; 18 / 71 / 47 under optimal decay with
# p_sb = 1, every -2 a collision).
RUNS = {
    "cbf_k3": ("cbf_qp", 3, {}, False, 0),
    "cbf_k1": ("cbf_qp", 1, {}, False, 0),
    "cbf_k6": ("cbf_qp", 6, {}, False, 0),
    "cbf_k10": ("cbf_qp", 10, {}, False, 0),
    "od_p1": ("optimal_decay_cbf_qp", 10, P1, False, 0),
    "od_default_penalty": ("optimal_decay_cbf_qp", 10, {}, False, 0),
    "cbf_k3_moving": ("cbf_qp", 3, {}, True, 0),
    "od_p1_moving": ("optimal_decay_cbf_qp", 10, P1, True, 0),
}


def setup(name, io="f64", idx=None):
    ctrl, K, odp, dyn, seed = RUNS[name]
    X0, wps, obs = Q.scene(B, seed, moving=dyn)
    if idx is not None:
        X0, wps = X0[idx], wps[idx]
    cfg = dict(controller=ctrl, spec=dict(Q.SPEC), param=odp, num_constraints=K, dt=0.05, dyn_obs=dyn)
    spec = dict(Q.SPEC, num_constraints=K, **{"cbf_" + k: v for k, v in odp.items()})
    ctl = sca.BatchedTrackingController(X0, spec, controller_type={"pos": ctrl}, dt=0.05, obs=obs, dyn_obs=dyn, io_dtype=io)
    assert type(ctl) is sca.tracking.BatchedQuadTrackingController and ctl.mpc is None
    ctl.set_waypoints(list(wps))
    return ctl, cfg, X0, wps, obs


def rollout(ctl, launches):
    od = ctl.od_qp
    out = [[], [], []]
    for n in launches:
        res = ctl.control_step(n, record=True)
        assert len(res) == (4 if od else 3)                      # (ret, traj_X, traj_U) and, under optimal decay, traj_omega
        for o, t in zip(out, res[1:]):
            o.append(t.double().cpu().numpy())
    return [np.concatenate(o) if o else None for o in out]


def compare(ctl, traj, r, tol, steps, full):
    """Trajectories up to each kept agent's last oracle step; with `full` also the final ret / ret_step / state machine / goal index
    (and omega / min_h under optimal decay)."""
    tX, tU, tW = traj
    keep = r["min_margin"] >= TIE
    assert (~keep).mean() <= 0.02, f"{int((~keep).sum())} agents within {TIE} of a selection tie"
    assert int(r["rejected_feasible"].sum()) == 0, "the oracle left its range of validity on this scene"
    n = np.minimum(r["n"], steps)
    valid = (np.arange(steps)[None, :] < n[:, None]) & keep[:, None]                    # [B, steps]
    pairs = [("X", tX, r["X"]), ("U", tU, r["U"])] + ([("omega", tW, r["W"])] if ctl.od_qp else [])
    for name, got, want in pairs:
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
    assert np.array_equal(ctl.state_machine.cpu().numpy()[k], r["sm_final"][k])
    assert np.array_equal(ctl.current_goal_index.cpu().numpy()[k], r["wp_final"][k])
    np.testing.assert_allclose(ctl.X.cpu().numpy()[k], r["X"][k, r["n"][k] - 1], rtol=tol, atol=tol)
    if ctl.od_qp:
        np.testing.assert_allclose(ctl.min_h.double().cpu().numpy()[k], r["min_h"][k], rtol=tol, atol=tol)
        np.testing.assert_allclose(ctl.omega.double().cpu().numpy()[k], r["W"][k, r["n"][k] - 1], rtol=tol, atol=tol)
    return keep


@pytest.mark.parametrize("name", list(RUNS))
def test_oracle_parity_f64(name):
    """120 steps in launches of 37 + 83 against the oracle at rtol = atol = 1e-6, the figure every fused-loop test here uses."""
    ctl, cfg, X0, wps, obs = setup(name)
    assert (ctl.n_wp.cpu().numpy() == 2).all() and (ctl.state_machine.cpu().numpy() == _lib.SM_TRACK).all()
    assert ctl.steps_done == 0
    traj = rollout(ctl, LAUNCHES)
    assert ctl.steps_done == T
    r = Q.run_many(cfg, X0, wps, obs, T)
    assert (r["sm0"] == Q.SM_INDEX["track"]).all()               # is_in_fov is always true for Quad2D
    keep = compare(ctl, traj, r, 1e-6, T, full=True)
    # not vacuous: finished, failed and still running; under 'cbf_qp' some failures are infeasible QPs; with p_sb = 1 the decay moved
    ret = r["ret"][keep]
    assert (ret == -1).any() and (ret == -2).any() and (ret == 0).any()
    assert (r["n"][keep] < LAUNCHES[0]).any() and ((r["n"][keep] > LAUNCHES[0]) & (ret != 0)).any()       # frozen before and after the boundary
    if cfg["controller"] == "cbf_qp":
        assert (r["infeasible"][keep] & (ret == -2)).any()
        assert not hasattr(ctl, "omega") and not hasattr(ctl, "min_h")
    elif cfg["param"] == P1:
        moved = np.nanmax(np.abs(r["W"] - 1.0), axis=(1, 2))
        assert (moved[keep] > 1e-3).any()
    if cfg["dyn_obs"]:
        want = obs.copy()
        for _ in range(T):
            want[:, 0:2] += want[:, 3:5] * 0.05
        np.testing.assert_allclose(ctl.obs.cpu().numpy(), want, rtol=0, atol=1e-12)
    else:
        assert np.array_equal(ctl.obs.cpu().numpy(), obs)


@pytest.mark.parametrize("name", ["cbf_k3", "cbf_k6", "cbf_k10", "od_p1", "cbf_k3_moving", "od_p1_moving"])
def test_oracle_parity_f32_storage_first_launch(name):
    """f32 storage, f64 arithmetic: the first launch against the oracle run from the states, waypoints and table re-read from the
    device, at 3e-6 as tests/test_tracking_od_gpu.py does.  K = 3, 6 and 10: the kernels built for up to 4, 8 and 16 rows."""
    ctl, cfg, _, _, _ = setup(name, io="f32")
    assert ctl.X.dtype == torch.float32 and ctl.obs.dtype == torch.float32
    X0 = ctl.X.double().cpu().numpy()
    obs = ctl.obs.double().cpu().numpy()
    assert (ctl.n_wp.cpu().numpy() == 2).all()                   # every route of the scene keeps both waypoints
    wps = ctl.waypoints.double().cpu().numpy()
    traj = rollout(ctl, LAUNCHES[:1])
    r = Q.run_many(cfg, X0, wps, obs, LAUNCHES[0])
    keep = compare(ctl, traj, r, 3e-6, LAUNCHES[0], full=False)
    assert keep.sum() >= 0.98 * B and (r["n"] < LAUNCHES[0]).any()


def big_table(obs):
    """The scene's rows, then small circles 500 m away up to 1171 rows: 65 576 B of LDS, the first table above the 64 KiB a kernel
    gets without the raised limit.  f32 numbers, so both storage types read the same table."""
    far = np.zeros((1171 - len(obs), 7))
    far[:, 0], far[:, 1], far[:, 2] = 500.0 + np.arange(len(far)), 500.0, 0.25
    return np.vstack([obs, far]).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("io,tol", [("f64", 1e-6), ("f32", 3e-6)])           # the figures of the two parity tests above
@pytest.mark.parametrize("name", ["cbf_k3", "cbf_k6", "cbf_k10", "od_p1"])
def test_table_above_64_kib_of_lds(name, io, tol):
    """M = 1171 rows, 3 agents, 2 steps in one launch against the oracle: the optimal-decay kernel and the CBF-QP kernels for up to 4,
    8 and 16 rows with the raised dynamic-LDS limit."""
    ctrl, K, odp, dyn, seed = RUNS[name]
    X0, wps, obs = Q.scene(B, seed, moving=dyn)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    X0, wps, obs = f32(X0[:3]), f32(wps[:3]), big_table(obs)
    cfg = dict(controller=ctrl, spec=dict(Q.SPEC), param=odp, num_constraints=K, dt=0.05, dyn_obs=dyn)
    spec = dict(Q.SPEC, num_constraints=K, **{"cbf_" + k: v for k, v in odp.items()})
    ctl = sca.BatchedTrackingController(X0, spec, controller_type={"pos": ctrl}, dt=0.05, obs=obs, dyn_obs=dyn, io_dtype=io)
    ctl.set_waypoints(list(wps))
    assert ctl.obs.shape[0] * 56 > 64 * 1024
    traj = rollout(ctl, (2,))
    r = Q._run_slice(cfg, X0, wps, obs, 2)
    keep = compare(ctl, traj, r, tol, 2, full=(io == "f64"))
    assert keep.all()


def quadtrack_select(ctl, K):
    """sc_quadtrack_select_batch on copies of the controller's state: (obs_sel [B,K,7], u_ref [B,2], track [B])."""
    rs = ctl.robot_spec
    p = _lib.QuadTrackParams()
    p.model, p.io_dtype, p.max_waypoints, p.waypoints_shared = 0, _lib.DTYPE_F64, int(ctl.waypoints.shape[1]), 0
    p.enable_rotation, p.num_constraints = 1, K
    p.dt, p.reached_threshold, p.rotation_threshold, p.robot_radius = 0.05, ctl.reached_threshold, ctl.rotation_threshold, float(rs["radius"])
    p.mass, p.inertia, p.f_min, p.f_max = float(rs["mass"]), float(rs["inertia"]), float(rs["f_min"]), float(rs["f_max"])
    t64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=DEV)
    n = ctl.B
    wps3, goal4 = t64(n, ctl.waypoints.shape[1], 3), t64(n, 4)
    wps3[:, :, :2] = ctl.waypoints
    goal4[:, :2], goal4[:, 3] = ctl.goal[:, :2], ctl.goal[:, 2]
    obs_sel, goal2, u_ref, track = t64(n, K, 7), t64(n, 2), t64(n, 2), torch.zeros(n, dtype=torch.int32, device=DEV)
    wp_i, sm = ctl.current_goal_index.clone(), ctl.state_machine.clone()
    rc = _lib.load().sc_quadtrack_select_batch(C.byref(p), n, int(ctl.obs.shape[0]), ctl.X.data_ptr(), wps3.data_ptr(), ctl.n_wp.data_ptr(),
                                               wp_i.data_ptr(), sm.data_ptr(), goal4.data_ptr(), ctl.obs.data_ptr(), ctl.ret.data_ptr(),
                                               obs_sel.data_ptr(), goal2.data_ptr(), u_ref.data_ptr(), track.data_ptr(), None)
    _lib.check(rc, "sc_quadtrack_select_batch")
    return obs_sel, u_ref, track


def test_one_step_equals_select_then_single_solve_cbf_qp():
    """For agents in 'track', the input of a one-step rollout is the composition of existing calls -- the only way to fly this on the
    parent commit: sc_quadtrack_select_batch, then BatchedCBFQP.solve (Quad2D) on the rows and reference it returns."""
    ctl, cfg, X0, wps, obs = setup("cbf_k3")
    ctl.control_step(20)                                         # away from the start: some rows are active, some QPs infeasible
    obs_sel, u_ref, track = quadtrack_select(ctl, 3)
    solver = sca.BatchedCBFQP(dict(ctl.robot_spec), dt=0.05, io_dtype="f64", compute_dtype="f64", cbf_param=dict(ctl.cbf_param))
    u, st, h = solver.solve(ctl.X.clone(), u_ref, obs_sel)
    before = ctl.ret.clone()
    ret, tX, tU = ctl.control_step(1, record=True)
    live = ((track != 0) & (before == 0)).cpu().numpy()
    ok = live & (st == _lib.STATUS_OPTIMAL).cpu().numpy()
    assert ok.sum() >= B // 2
    np.testing.assert_allclose(tU.cpu().numpy()[0][ok], u.cpu().numpy()[ok], rtol=0, atol=1e-12)
    assert (np.abs(u.cpu().numpy()[ok] - u_ref.cpu().numpy()[ok]).max(axis=1) > 1e-3).any()      # the barrier moved some inputs
    bad = live & ~ok
    assert (ret.cpu().numpy()[bad] == -2).all()                  # a non-optimal single solve is a -2 of the loop


def test_one_step_equals_select_then_single_solve_od():
    """Under optimal decay: sc_quadtrack_select_batch with one row, then BatchedOptimalDecayCBFQP.solve; omega and min_h as well."""
    ctl, cfg, X0, wps, obs = setup("od_p1")
    obs_sel, u_ref, track = quadtrack_select(ctl, 1)
    solver = sca.BatchedOptimalDecayCBFQP(dict(ctl.robot_spec), dt=0.05, io_dtype="f64", compute_dtype="f64", cbf_param=dict(ctl.cbf_param))
    u, w, st, h = solver.solve(ctl.X.clone(), u_ref, obs_sel[:, 0].contiguous())
    ret, tX, tU, tW = ctl.control_step(1, record=True)
    m = ((track != 0) & (ret == 0) & (st == _lib.STATUS_OPTIMAL)).cpu().numpy()
    assert m.sum() >= B // 2
    np.testing.assert_allclose(tU.cpu().numpy()[0][m], u.cpu().numpy()[m], rtol=0, atol=1e-12)
    np.testing.assert_allclose(tW.cpu().numpy()[0][m], w.cpu().numpy()[m], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ctl.omega.cpu().numpy()[m], w.cpu().numpy()[m], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ctl.min_h.cpu().numpy()[m], h.cpu().numpy()[m], rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ["cbf_k3_moving", "od_p1_moving"])
def test_moving_table_every_block_sees_the_same_table(name):
    """4096 agents (64 blocks) over a moving table in two launches: every block reads the table as it was at launch and advances its
    own copy, so the 30 copies of each of the scene's 136 agents, which sit in different blocks and lanes, stay bit-identical, agent
    0 matches a run on its own, and the table ends where n steps of obs += v dt put it."""
    n_big, launches = 4096, (25, 35)
    idx = np.arange(n_big) % B
    big, _, _, _, obs = setup(name, idx=idx)
    one, _, _, _, _ = setup(name, idx=np.arange(1))
    for n in launches:
        big.control_step(n)
        one.control_step(n)
    for a in ("X", "ret", "ret_step", "u_pos", "state_machine", "current_goal_index") + (("omega", "min_h") if big.od_qp else ()):
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


@pytest.mark.parametrize("ctrl", Q.CONTROLLERS)
def test_no_obstacles_matches_the_oracle(ctrl):
    """obs=None: 'cbf_qp' passes u_ref through unsolved (cbf_qp.py:113-118), optimal decay still solves, with a zero row, and leaves
    omega at its reference and min_h at +inf.  Both against the oracle over a short climb that ends in -1."""
    X0 = np.array([[0.0, 0.2, 0.05, 0.1, 0.3, 0.0], [1.0, 0.5, -0.05, 0.0, 0.0, 0.1]])
    wps = np.array([[[0.02, 0.55], [0.0, 0.9]], [[1.0, 3.0], [1.2, 5.0]]])
    ctl = sca.BatchedTrackingController(X0, dict(Q.SPEC), controller_type={"pos": ctrl}, obs=None)
    ctl.set_waypoints(list(wps))
    res = ctl.control_step(80, record=True)
    tX, tU = res[1].cpu().numpy(), res[2].cpu().numpy()
    cfg = dict(controller=ctrl, spec=dict(Q.SPEC))
    for i in range(2):
        r = Q.run(Q.make_oracle(cfg, X0[i], wps[i], None), 80)
        n = len(r["X"])
        np.testing.assert_allclose(tX[:n, i], r["X"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(tU[:n, i], r["U"], rtol=1e-6, atol=1e-6)
        assert int(ctl.ret[i].item()) == r["ret"] == (-1 if i == 0 else 0)
        assert np.array_equal(tX[n:, i], np.broadcast_to(tX[n - 1, i], tX[n:, i].shape))       # a frozen agent repeats its last state
    if ctrl == "optimal_decay_cbf_qp":
        assert np.array_equal(res[3].cpu().numpy(), np.ones((80, 2, 2))) and np.isinf(ctl.min_h.cpu().numpy()).all()


def test_refusals():
    """A superellipsoid row is refused under the two QP controllers (Quad2D.agent_barrier has no such branch), at construction and in
    set_obstacles; Quad3D and VTOL2D keep raising for them; the default controller of Quad2D stays 'mpc_cbf'."""
    X0 = np.zeros((2, 2))
    se = np.array([[1.0, 2.0, 0.3, 0.0, 0.0, 0.0, 0.0], [2.4, 3.0, 0.45, 0.25, 4.0, 0.4, 1.0]])
    for ctrl in Q.CONTROLLERS:
        with pytest.raises(ValueError, match="superellipsoid"):
            sca.BatchedTrackingController(X0, dict(Q.SPEC), controller_type={"pos": ctrl}, obs=se)
        ctl = sca.BatchedTrackingController(X0, dict(Q.SPEC), controller_type={"pos": ctrl}, obs=se[:1])
        with pytest.raises(ValueError, match="superellipsoid"):
            ctl.set_obstacles(se)
        for model in ("Quad3D", "VTOL2D"):
            with pytest.raises(ValueError):
                sca.BatchedTrackingController(X0, {"model": model}, controller_type={"pos": ctrl})
    with pytest.raises(ValueError):
        sca.BatchedTrackingController(X0, dict(Q.SPEC, num_constraints=17), controller_type={"pos": "cbf_qp"})
    with pytest.raises(ValueError):
        sca.BatchedTrackingController(X0, dict(Q.SPEC), controller_type={"pos": "optimal_decay_mpc_cbf"})
    with pytest.raises(ValueError):                              # moving tables stay with the fused rollouts
        sca.BatchedTrackingController(X0, dict(Q.SPEC), dyn_obs=True)
    dflt = sca.BatchedTrackingController(X0, dict(Q.SPEC), obs=se)                               # 'mpc_cbf' takes the table as before
    assert dflt.pos_controller_type == "mpc_cbf" and dflt.mpc is not None and dflt.goal.shape == (2, 4)
