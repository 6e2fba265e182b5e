"""GPU: csrc/mpc_du_ms.hip (kernel 13) -- the DynamicUnicycle2D MPC-CBF NLP as do-mpc poses it (multiple shooting) under IPOPT's filter interior
point, one NLP per wavefront -- against oracle/ms_ipopt.py with du_model() in the kernel's profile (Riccati linear algebra, no second-order
corrections, restoration phase with elastic variables on the CBF rows, stall rule): SAME STATUS and SAME ITERATION COUNT problem by problem
(at most 2 % may differ by an iteration or two at the tolerance), |u0 - u0_oracle| <= 1e-8 -- on the ~10 % of BASELINE configs[2] draws that
have no feasible point as well: there the returned input is the restoration phase's last iterate, which is what the reference applies
(position_control/mpc_cbf.py:384, status hard-wired 'optimal', :10)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import safe_control_amd as sca  # noqa: E402
from safe_control_amd import _lib, workloads as W  # noqa: E402
from oracle import ms_ipopt as MS  # noqa: E402
from _oracle_pool import ms_batch, ms_cached, ms_solve_many, take  # noqa: E402

DEV = "cuda:0"
PROFILE = dict(MS.KERNEL13_PROFILE)
SPEC = {"model": "DynamicUnicycle2D", "a_max": 1.0, "w_max": 0.5, "v_max": 1.0, "radius": 0.25}


def t(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def oracle_many(X, up, goal, obs, N=None):
    """oracle/ms_ipopt.py on every row, in the host's child-process pool (tests/_oracle_pool.py)."""
    return ms_solve_many("du", X, up, goal, obs, opts=PROFILE, N=N, spec=SPEC)


def oracle_draws(seed, n):
    """The first n problems of the seed's bench batch and the oracle's solves of them: seed 0 from the session's run over all 4096
    (tests/test_mpccbf_ms_full_batch_gpu.py reads the same), other seeds solved here."""
    if seed == 0:
        (X, up, goal, obs), r = ms_batch("du", 0, opts=PROFILE, spec=SPEC)
        return (X[:n], up[:n], goal[:n], obs[:n]), take(r, slice(0, n))
    X, up, goal, obs = (a[:n] for a in W.mpc_family_batch("du", 4096, 8, seed=seed))
    return (X, up, goal, obs), ms_cached("du", ("mpc_family_batch", seed, 4096, 8, "head", n), X, up, goal, obs, opts=PROFILE, spec=SPEC)


def compare(u, st, it, plan, res, n_off):
    so, ito = res["st"], res["it"]
    assert np.array_equal(st, so), np.flatnonzero(st != so)[:10]
    off = it != ito
    assert off.sum() <= n_off and np.abs(it - ito).max() <= 2, (int(off.sum()), int(np.abs(it - ito).max()))
    du = np.abs(u - res["u"]).max(axis=1)
    assert du[~off].max() <= 1e-8 and du.max() <= 1e-6, (du[~off].max(), du.max())                # every status: the infeasible solves' iterate too
    if plan is not None:
        dp = np.abs(plan - res["plan"]).max(axis=1)
        ok = so == 0
        assert dp[ok & ~off].max() <= 1e-6 and dp[~off].max() <= 1e-5, (dp[ok & ~off].max(), dp[~off].max())      # (2e-7 seen: weakly determined headings far down the horizon)
    return so, ito


@pytest.mark.parametrize("seed", [0, 3])
def test_config3_draws_against_the_oracle_iterate_for_iterate(seed):
    n = 384
    (X, up, goal, obs), res = oracle_draws(seed, n)
    ctl = sca.BatchedMSMPCCBF(SPEC, io_dtype="f64")
    u, st, it, plan, trace = ctl.solve(t(X), t(up), t(goal), t(obs), want_plan=True, want_trace=True)
    torch.cuda.synchronize()
    u, st, it, plan, trace = (a.cpu().numpy() for a in (u, st, it, plan, trace))
    so, ito = compare(u, st, it, plan, res, n_off=8)
    assert 0.02 <= (so == 1).mean() <= 0.2 and (so == 2).mean() <= 0.01          # the infeasible draws are in the sample: restoration phase, certificate
    worst = 0.0
    for i in range(n):
        T = res["trace"][i]                                                      # (the oracle's first TRACE_ROWS trace rows, ntr in all)
        m = min(int(res["ntr"][i]), it[i] + 1, 12)
        in_resto = np.flatnonzero(np.signbit(T[:, 7]))                                  # (the oracle's restoration writes a row of its own when it starts: rows before it)
        m = min(m, in_resto[0] - 1) if len(in_resto) else m                      # (and the kernel writes its restoration start row over the row of the iterate it starts from)
        worst = max(worst, float((np.abs(trace[i, :m, :6] - T[:m, :6]) / np.maximum(1e-7, np.abs(T[:m, :6]))).max()))
    assert worst <= 1e-5, worst
    print(f"du ms kernel: optimal {np.mean(so == 0):.4f}, infeasible {np.mean(so == 1):.4f}, iterations mean {ito.mean():.1f} max {ito.max()}, equal on {np.mean(it == ito):.4f}")


def test_full_batch_properties_and_the_condensed_kernel_on_the_feasible_draws():
    """All 4096 configs[2] problems: launch twice -> bitwise equal; every returned input inside the box; where this kernel and the condensed one
    (kernel 3) both end optimal they hold the same optimum on >= 99.5 % (the NLP is non-convex: a handful of other local optima, 8 of 3658
    between the two oracles)."""
    X, up, goal, obs = W.mpc_family_batch("du", 4096, 8, seed=0)
    f = lambda a: t(a.astype(np.float32), torch.float32)                          # noqa: E731
    ctl = sca.BatchedMSMPCCBF(SPEC, io_dtype="f32")
    u1, s1, i1 = ctl.solve(f(X), f(up), f(goal), f(obs))
    u2, s2, i2 = ctl.solve(f(X), f(up), f(goal), f(obs))
    assert torch.equal(u1, u2) and torch.equal(s1, s2) and torch.equal(i1, i2)
    # the launch order (problems whose start violates a CBF row first: a pre-pass + a permutation of the grid) changes the launch time only
    u3, s3, i3 = sca.BatchedMSMPCCBF(SPEC, io_dtype="f32", order=False).solve(f(X), f(up), f(goal), f(obs))
    assert torch.equal(u1, u3) and torch.equal(s1, s3) and torch.equal(i1, i3)
    assert (u1[:, 0].abs() <= 1.0 + 1e-6).all() and (u1[:, 1].abs() <= 0.5 + 1e-6).all()
    opt = (s1 == 0).double().mean().item()
    assert 0.85 <= opt <= 0.93 and (s1 == 2).double().mean().item() <= 0.005, opt
    uc, sc, ic = sca.BatchedMPCCBF(SPEC, io_dtype="f32").solve(f(X), f(up), f(goal), f(obs))
    both = (s1 == 0) & (sc == 0)
    same = ((u1 - uc).abs().amax(dim=1) <= 1e-4)[both].double().mean().item()
    assert both.double().mean().item() >= 0.85 and same >= 0.995, (both.double().mean().item(), same)
    print(f"du ms kernel, 4096: optimal {opt:.4f}, iterations mean {i1.double().mean().item():.1f} max {int(i1.max())}; same optimum as the condensed kernel on {same:.4f}")


def test_f32_storage_shared_obstacles_sixteen_slots_and_a_longer_horizon():
    n = 64
    X, up, goal, obs = (a[:n] for a in W.mpc_family_batch("du", 64, 10, seed=5))
    ctl = sca.BatchedMSMPCCBF(SPEC, io_dtype="f64")
    u, st, it = (a.cpu().numpy() for a in ctl.solve(t(X), t(up), t(goal), t(obs)))
    compare(u, st, it, None, oracle_many(X, up, goal, obs), n_off=2)
    # horizon 20 (BASELINE configs[4] runs N = 20)
    c20 = sca.BatchedMSMPCCBF(SPEC, io_dtype="f64", horizon=20)
    u, st, it = (a.cpu().numpy() for a in c20.solve(t(X[:32]), t(up[:32]), t(goal[:32]), t(obs[:32])))
    compare(u, st, it, None, oracle_many(X[:32], up[:32], goal[:32], obs[:32], N=20), n_off=2)
    # f32 storage of f32-representable inputs = the f64 solve of the same numbers, rounded on the way out; one obstacle table for everybody
    X32, up32, goal32 = (a.astype(np.float32) for a in (X, up, goal))
    ob32 = np.ascontiguousarray(obs[0]).astype(np.float32)
    ob32[:, :2] += 30.0
    c32 = sca.BatchedMSMPCCBF(SPEC, io_dtype="f32")
    u32, s32, i32 = c32.solve(t(X32, torch.float32), t(up32, torch.float32), t(goal32, torch.float32), t(ob32, torch.float32))
    u64, s64, i64 = ctl.solve(t(X32.astype(np.float64)), t(up32.astype(np.float64)), t(goal32.astype(np.float64)), t(ob32.astype(np.float64)))
    assert torch.equal(s32, s64) and torch.equal(i32, i64) and torch.equal(u32, u64.float())


def test_argument_validation_and_superellipsoid_rows():
    lib = _lib.load()
    import ctypes as C
    from safe_control_amd.position_control import mpc_cbf as PM
    from safe_control_amd.robots.spec import complete_robot_spec
    sp = complete_robot_spec(dict(SPEC))
    Q, R = PM.default_mpc_weights("DynamicUnicycle2D")
    p = PM.make_params(sp, PM.default_mpc_cbf_param("DynamicUnicycle2D"), Q, R, 10, 0.05, sp["radius"], _lib.DTYPE_F64)
    ip = _lib.default_ipopt()
    none10 = [None] * 10
    assert lib.sc_mpccbf_ms_solve_batch(C.byref(p), C.byref(ip), 0, 8, *none10) == _lib.SC_OK
    assert lib.sc_mpccbf_ms_solve_batch(C.byref(p), C.byref(ip), 1, 8, *none10) != _lib.SC_OK            # NULL buffers
    assert lib.sc_mpccbf_ms_solve_batch(C.byref(p), C.byref(ip), 0, 17, *none10) != _lib.SC_OK
    assert lib.sc_mpccbf_ms_solve_batch(C.byref(p), None, 0, 8, *none10) != _lib.SC_OK
    assert lib.sc_mpccbf_ms_solve_batch(C.byref(p), C.byref(_lib.default_ipopt(tau_min=1.5)), 0, 8, *none10) != _lib.SC_OK
    assert lib.sc_mpccbf_ms_solve_batch(C.byref(p), C.byref(_lib.default_ipopt(resto_penalty_parameter=0.0)), 0, 8, *none10) != _lib.SC_OK
    p.horizon = 63
    assert lib.sc_mpccbf_ms_solve_batch(C.byref(p), C.byref(ip), 0, 8, *none10) != _lib.SC_OK
    p.horizon = 10
    p.model_id = _lib.MODEL_IDS["Quad2D"]                                       # (served: DynamicUnicycle2D, Unicycle2D, DoubleIntegrator2D, KinematicBicycle2D)
    assert lib.sc_mpccbf_ms_solve_batch(C.byref(p), C.byref(ip), 0, 8, *none10) != _lib.SC_OK
    p.model_id = _lib.MODEL_IDS["KinematicBicycle2D"]; p.rear_ax_dist = 0.0     # (the bicycle needs its L_r)
    assert lib.sc_mpccbf_ms_solve_batch(C.byref(p), C.byref(ip), 0, 8, *none10) != _lib.SC_OK
    assert int(lib.sc_mpccbf_ms_lds_bytes(10, 8)) > 0 and int(lib.sc_mpccbf_ms_lds_bytes(10, 17)) == 0
    X, up, goal, obs = (a[:4] for a in W.mpc_family_batch("uni", 4, 8, seed=0))
    obs = obs.copy(); obs[2, 3] = [4.0, 4.0, 0.6, 0.4, 4.0, 0.3, 1.0]
    with pytest.raises(NotImplementedError):                                    # (Unicycle2D's DT barrier has no superellipsoid branch; tests/test_mpccbf_ms_se_gpu.py: the robots that have)
        sca.BatchedMSMPCCBF({"model": "Unicycle2D"}, io_dtype="f64").solve(t(X), t(up), t(goal), t(obs))
    p.model_id = _lib.MODEL_IDS["KinematicBicycle2D"]; p.rear_ax_dist = 0.2; p.superellipsoid_rows = 1
    assert lib.sc_mpccbf_ms_solve_batch(C.byref(p), C.byref(ip), 0, 8, *none10) != _lib.SC_OK
    with pytest.raises(NotImplementedError):
        sca.BatchedMSMPCCBF({"model": "Quad2D"})


def test_dropin_class_closed_loop_follows_the_multiple_shooting_oracle():
    """MPCCBF through the reference's plugin surface (the default formulation of a DynamicUnicycle2D robot since round 6), 15 closed-loop steps
    with u_prev feedback against oracle/ms_ipopt.py; 'condensed' stays selectable; a superellipsoid row in the scene selects the kernel's superellipsoid instantiation."""
    from oracle import robots as R, mpc_cbf as M
    robot = sca.RobotHandle(np.array([2.0, 2.0, np.pi / 2, 1.0]), dict(SPEC), dt=0.05)
    ctl = sca.MPCCBF(robot, dict(SPEC), num_obs=8)
    assert ctl._ms is not None
    obs = [[2.2, 5.0, 0.2], [3.0, 5.0, 0.2], [4.0, 9.0, 0.3]]
    goal = np.array([2.0, 12.0])
    Xo = robot.X.reshape(-1).copy(); up = np.zeros(2)
    ospec = R.default_spec(R.MODEL_DU); ospec.update(a_max=1.0, w_max=0.5)
    for k in range(15):
        u = ctl.solve_control_problem(robot.X, {"state_machine": "track", "u_ref": np.zeros((2, 1)), "goal": goal}, obs)
        uo, so, ito = MS.solve(MS.du_model(), Xo, up, goal, M.pad_obstacles(obs, 8), opts=PROFILE)
        assert u.shape == (2, 1) and ctl.status == "optimal" and ctl.solver_status == "optimal" and so == 0 and ctl.iterations == ito
        np.testing.assert_allclose(u.reshape(-1), uo, atol=1e-8)
        assert ctl.z.shape == (20,) and np.abs(ctl.z[:2] - uo).max() <= 1e-8
        Xo = R.step(R.MODEL_DU, Xo, uo, 0.05, ospec); up = uo
        robot.X = R.step(R.MODEL_DU, robot.X.reshape(-1), u.reshape(-1), 0.05, ospec).reshape(-1, 1)
    ur = np.array([[0.3], [-0.1]])
    assert ctl.solve_control_problem(robot.X, {"state_machine": "stop", "u_ref": ur, "goal": goal}, obs) is ur      # mpc_cbf.py:379-381
    with pytest.raises(ValueError):
        ctl.solve_control_problem(robot.X, {"state_machine": "track", "u_ref": ur, "goal": goal}, [[1.0, 2.0, 0.3, 0.0, 0.0]])
    cond = sca.MPCCBF(sca.RobotHandle(np.array([2.0, 2.0, np.pi / 2, 1.0]), dict(SPEC), dt=0.05), dict(SPEC, mpc_formulation="condensed"), num_obs=8)
    assert cond._ms is None
    se = obs + [[6.0, 6.0, 0.6, 0.4, 4.0, 0.3, 1.0]]
    x0 = np.array([2.0, 2.0, np.pi / 2, 1.0])
    ctl.u_prev = np.zeros(2)
    u_se = ctl.solve_control_problem(x0.reshape(-1, 1), {"state_machine": "track", "u_ref": np.zeros((2, 1)), "goal": goal}, [o + [0.0] * (7 - len(o)) for o in se])
    pad = M.pad_obstacles([o + [0.0] * (7 - len(o)) for o in se], 8)
    um, sm, _ = MS.solve(MS.du_model(), x0, np.zeros(2), goal, pad, opts=PROFILE)                # (kernel 13's superellipsoid instantiation: csrc/mpc_du_ms_se.hip)
    assert sm == 0 and ctl._ms.superellipsoids is True and np.abs(u_se.reshape(-1) - um).max() <= 1e-8
    uo, so, _ = M.solve(x0, np.zeros(2), goal, pad)                                               # (the condensed oracle: the same optimum)
    assert so == 0 and np.abs(u_se.reshape(-1) - uo).max() <= 1e-5
