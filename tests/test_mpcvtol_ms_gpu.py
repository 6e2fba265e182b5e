"""GPU: csrc/mpc_vtol_ms.hip -- the VTOL2D MPC-CBF NLP as do-mpc poses it (multiple shooting), IPOPT's filter interior point, one NLP per
wavefront -- against oracle/ms_ipopt.py in the kernel's profile (Riccati linear algebra, no second-order corrections, restoration phase with
elastic variables on the CBF rows, stall rule): SAME STATUS and SAME ITERATION COUNT problem by problem (at most 3 % may differ by one iteration at the
tolerance), |u0 - u0_oracle| <= 1e-8 (1e-7 on those), plans (positions of ~100 m, weakly determined far down the horizon) to 1e-5; the traces of the two solvers (E_0, infeasibilities, mu, theta, delta_w, alpha per
iteration) agree to 1e-5 relative over the first 15 iterations.  Then the restoration phase inside the kernel against the oracle's, the hand-over to
the condensed kernel when no workspace is given, f32 storage, shared obstacles, 16 row slots, the optimal-decay instantiation."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import safe_control_amd as sca  # noqa: E402
from safe_control_amd import _lib, workloads as W  # noqa: E402
from oracle import ms_ipopt as MS  # noqa: E402
from _oracle_pool import ms_solve_many  # noqa: E402

DEV = "cuda:0"
PROFILE = dict(MS.KERNEL_PROFILE)                  # what the kernel runs: Riccati linear algebra, no second-order corrections, restoration on the CBF rows, stall rule


def t(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def oracle_many(X, up, goal, obs, spec=None, opts=None):
    """oracle/ms_ipopt.py on every row in the host's child-process pool (tests/_oracle_pool.py): per row (u, status, iterations, the first
    iterates' trace [E0, dinf, pinf, comp, mu, theta, delta_w, alpha], plan)."""
    r = ms_solve_many("vtol", X, up, goal, obs, opts=opts or PROFILE, spec=spec)
    T = [r["trace"][i, :min(int(r["ntr"][i]), len(r["trace"][i]))].copy() for i in range(len(X))]
    for q in T:
        q[:, 7] = np.abs(q[:, 7])                                         # (this trace's step lengths are unsigned in the restoration, as the kernel's)
    return [(r["u"][i], r["st"][i], r["it"][i], T[i], r["plan"][i]) for i in range(len(X))]


def compare(u, st, it, plan, res, n_off=8):
    so, ito = np.array([r[1] for r in res]), np.array([r[2] for r in res])
    assert np.array_equal(st, so), np.flatnonzero(st != so)[:10]
    off = it != ito
    assert off.sum() <= n_off and np.abs(it - ito).max() <= 2, (int(off.sum()), int(np.abs(it - ito).max()))       # (one or two iterations more or less at tol = 1e-8)
    ok = so == 0
    du = np.array([np.abs(u[i] - r[0]).max() for i, r in enumerate(res)])
    assert du[ok & ~off].max() <= 1e-8 and du[ok].max() <= 1e-7, (du[ok & ~off].max(), du[ok].max())      # (one iteration more or less at tol = 1e-8)
    if plan is not None:
        dp = np.array([np.abs(plan[i] - r[4]).max() for i, r in enumerate(res)])
        assert dp[ok & ~off].max() <= 1e-5 and dp[ok].max() <= 5e-5, (dp[ok & ~off].max(), dp[ok].max())     # (states of ~100 m: 1e-7 relative)
    return so, ito


@pytest.mark.parametrize("seed", [0, 1])
def test_batch_against_the_oracle_iterate_for_iterate(seed):
    n = 256
    X, up, goal, obs = (a[:n] for a in W.mpc_family_batch("vtol", 4096, 8, seed=seed))
    ctl = sca.BatchedVtolMSMPCCBF(io_dtype="f64", fallback=False)
    u, st, it, plan, trace = ctl.solve(t(X), t(up), t(goal), t(obs), want_plan=True, want_trace=True)
    torch.cuda.synchronize()
    u, st, it, plan, trace = (a.cpu().numpy() for a in (u, st, it, plan, trace))
    res = oracle_many(X, up, goal, obs)
    so, ito = compare(u, st, it, plan, res)
    assert (so == 0).mean() >= 0.98
    worst = 0.0
    for i, r in enumerate(res):
        m = min(len(r[3]), it[i] + 1, 15)
        worst = max(worst, float((np.abs(trace[i, :m] - r[3][:m]) / np.maximum(1e-9, np.abs(r[3][:m]))).max()))
    assert worst <= 1e-5, worst                                           # (first 15 iterations; the recursion sums in the order of the MFMA)
    print(f"ms kernel: optimal {np.mean(so == 0):.4f}, iterations mean {ito.mean():.1f} max {ito.max()}, equal on {np.mean(it == ito):.4f}")


def test_sixteen_slots_f32_storage_shared_obstacles():
    n = 48
    X, up, goal, obs = (a[:n] for a in W.mpc_family_batch("vtol", 64, 10, seed=5))
    ctl = sca.BatchedVtolMSMPCCBF(io_dtype="f64", fallback=False)
    u, st, it = (a.cpu().numpy() for a in ctl.solve(t(X), t(up), t(goal), t(obs)))
    compare(u, st, it, None, oracle_many(X, up, goal, obs), n_off=3)
    # f32 storage of f32-representable inputs = the f64 solve of the same numbers, rounded on the way out
    X32, up32, goal32 = (a.astype(np.float32) for a in (X, up, goal))
    ob32 = np.ascontiguousarray(obs[0]).astype(np.float32)
    ob32[:, 0] += 40.0                                                      # one obstacle set for everybody, far enough ahead for all
    c32 = sca.BatchedVtolMSMPCCBF(io_dtype="f32", fallback=False)
    u32, s32, i32 = c32.solve(t(X32, torch.float32), t(up32, torch.float32), t(goal32, torch.float32), t(ob32, torch.float32))
    u64, s64, i64 = ctl.solve(t(X32.astype(np.float64)), t(up32.astype(np.float64)), t(goal32.astype(np.float64)), t(ob32.astype(np.float64)))
    assert torch.equal(s32, s64) and torch.equal(i32, i64)
    assert torch.equal(u32, u64.float())


SCENE_OBS = np.hstack([np.array([[67.0, z, 0.5] for z in (6.0, 7.0, 8.0, 9.0)] + [[73.0, float(z), 0.5] for z in range(1, 7)]), np.zeros((10, 4))])
SCENE_SPEC = {"model": "VTOL2D", "radius": 0.6, "v_max": 20.0}


def test_restoration_phase_against_the_oracle():
    """The first NLP of the reference's example scene has no feasible point (20 m/s towards a wall 65 m ahead, 15 degrees of pitch), nor have
    the NLPs a few metres further on: the line search ends below alpha_min after ~30 iterations and IPOPT's restoration phase takes over --
    inside the kernel (elastic variables on the CBF rows, its own filter, the return test against the regular filter), as in
    oracle/ms_ipopt.py with KERNEL_PROFILE.  Held: seven starts, same status on all (1 = converged to a point of local infeasibility:
    the certificate), same iteration count on five or more (measured: six; the seventh 155 against 161), same input where the counts
    agree (1e-8), 50 - 120 of each solve's iterations inside the restoration; a feasible problem in the same batch is untouched."""
    n = 7
    X = np.array([[2.0 + i, 10.0 - 0.05 * i, 0.0, 20.0, 0.0, 0.0] for i in range(n)] + [[2.0, 10.0, 0.0, 8.0, 0.0, 0.0]])
    goal = np.array([[70.0, 10.0]] * n + [[40.0, 10.0]])
    ob = np.stack([SCENE_OBS] * n + [np.tile(np.array([1000.0, 1000.0, 0, 0, 0, 0, 0]), (10, 1))])
    up = np.zeros((n + 1, 4))
    ctl = sca.BatchedVtolMSMPCCBF(SCENE_SPEC, io_dtype="f64", fallback=False)
    u, st, it, trace = (a.cpu().numpy() for a in ctl.solve(t(X), t(up), t(goal), t(ob), want_trace=True))
    res = oracle_many(X, up, goal, ob, spec=dict(radius=0.6, v_max=20.0))
    so, ito = np.array([r[1] for r in res]), np.array([r[2] for r in res])
    print("restoration: kernel", st.tolist(), it.tolist(), "oracle", so.tolist(), ito.tolist())
    assert np.array_equal(st, so) and st[:n].tolist() == [1] * n and st[n] == 0
    same = it == ito
    assert same.sum() >= 6 and np.abs(it - ito).max() <= 0.1 * ito.max()
    du = np.array([np.abs(u[i] - r[0]).max() for i, r in enumerate(res)])
    assert du[same].max() <= 1e-8, du
    in_resto = np.array([(trace[i, :it[i] + 1, 7] < 0).sum() for i in range(n + 1)])     # (a negative step length marks an iterate of the restoration)
    assert (in_resto[:n] >= 40).all() and in_resto[n] == 0, in_resto


def test_without_a_workspace_the_kernel_hands_restorations_back():
    """restoration = False (sc_ipopt_params.resto_workspace = NULL): SC_STATUS_NEEDS_RESTO at the iteration at which the oracle without a
    restoration phase stops, and the host class solves that problem with the condensed kernel, whose status and input it then carries."""
    X = np.array([[2.0, 10.0, 0.0, 20.0, 0.0, 0.0], [2.0, 10.0, 0.0, 8.0, 0.0, 0.0]])
    goal = np.array([[70.0, 10.0], [40.0, 10.0]])
    ob = np.stack([SCENE_OBS, np.tile(np.array([1000.0, 1000.0, 0, 0, 0, 0, 0]), (10, 1))])
    up = np.zeros((2, 4))
    raw = sca.BatchedVtolMSMPCCBF(SCENE_SPEC, io_dtype="f64", fallback=False, restoration=False)
    u, st, it = raw.solve(t(X), t(up), t(goal), t(ob))
    assert st.cpu().tolist() == [_lib.STATUS_NEEDS_RESTO, 0]
    res = oracle_many(X, up, goal, ob, spec=dict(radius=0.6, v_max=20.0), opts=dict(MS.KERNEL_PROFILE_NO_RESTO))
    assert [r[1] for r in res] == [4, 0] and [r[2] for r in res] == it.cpu().tolist()
    full = sca.BatchedVtolMSMPCCBF(SCENE_SPEC, io_dtype="f64", restoration=False)
    u2, st2, it2 = full.solve(t(X), t(up), t(goal), t(ob))
    assert full.n_fallback == 1 and int(st2[0]) in (1, 2) and int(st2[1]) == 0
    cond = sca.BatchedVtolMPCCBF(SCENE_SPEC, io_dtype="f64")
    uc, sc_, ic = cond.solve(t(X[:1]), t(up[:1]), t(goal[:1]), t(ob[:1]))
    assert torch.equal(u2[0], uc[0]) and int(st2[0]) == int(sc_[0]) and int(it2[0]) == int(it[0]) + int(ic[0])
    assert torch.equal(u2[1], u[1])


def test_argument_validation():
    lib = _lib.load()
    import ctypes as C
    from safe_control_amd.position_control.mpc_cbf_vtol import make_params, CBF_VTOL
    from safe_control_amd.robots.spec import complete_robot_spec
    sp = complete_robot_spec({"model": "VTOL2D"})
    p = make_params(sp, CBF_VTOL, 30, 0.05, sp["radius"], _lib.DTYPE_F64)
    ip = _lib.default_ipopt()
    assert lib.sc_mpcvtol_ms_solve_batch(C.byref(p), C.byref(ip), 0, 8, *([None] * 10)) == _lib.SC_OK
    assert lib.sc_mpcvtol_ms_solve_batch(C.byref(p), C.byref(ip), 1, 17, *([None] * 10)) != _lib.SC_OK
    assert lib.sc_mpcvtol_ms_solve_batch(C.byref(p), None, 1, 8, *([None] * 10)) != _lib.SC_OK
    bad = _lib.default_ipopt(tau_min=1.5)
    assert lib.sc_mpcvtol_ms_solve_batch(C.byref(p), C.byref(bad), 1, 8, *([None] * 10)) != _lib.SC_OK
    # a restoration workspace one byte short of sc_mpcvtol_ms_workspace_bytes(B, K) is refused by BOTH entry points before anything is
    # launched (the kernel indexes the workspace per problem without a bound check), and so are restoration options out of range
    from safe_control_amd.position_control.mpc_cbf_vtol import make_od_params, OD_CBF_VTOL
    pod = make_od_params(sp, OD_CBF_VTOL, 30, 0.05, sp["radius"], _lib.DTYPE_F64)
    need = int(lib.sc_mpcvtol_ms_workspace_bytes(4, 8))
    assert need == 4 * (8 * 8 + 12) * 64 * 8 and int(lib.sc_mpcvtol_ms_workspace_bytes(4, 9)) == 4 * (8 * 16 + 12) * 64 * 8
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    for short, kw in ((1, {}), (0, {"resto_penalty_parameter": 0.0}), (0, {"required_infeasibility_reduction": 1.0})):
        q = _lib.default_ipopt(**kw)
        q.resto_workspace, q.resto_workspace_bytes = ws.data_ptr(), need - short
        assert lib.sc_mpcvtol_ms_solve_batch(C.byref(p), C.byref(q), 4, 8, *([None] * 10)) == _lib.SC_ERR_INVALID_ARGUMENT
        assert lib.sc_odmpcvtol_ms_solve_batch(C.byref(pod), C.byref(q), 4, 8, *([None] * 11)) == _lib.SC_ERR_INVALID_ARGUMENT
    q = _lib.default_ipopt()
    q.resto_workspace, q.resto_workspace_bytes = ws.data_ptr(), need
    assert lib.sc_mpcvtol_ms_solve_batch(C.byref(p), C.byref(q), 0, 8, *([None] * 10)) == _lib.SC_OK
    p.horizon = 63
    assert lib.sc_mpcvtol_ms_solve_batch(C.byref(p), C.byref(ip), 1, 8, *([None] * 10)) != _lib.SC_OK


def oracle_od_many(X, up, goal, obs, N=30):
    """The optimal-decay oracle on every row: per row (u_0, status, iterations, decay rates of the plan, f, restoration iterates)."""
    r = ms_solve_many("vtol_od", X, up, goal, obs, opts=PROFILE)
    U = r["plan"][:, (N + 1) * 6:].reshape(len(X), N, -1)                 # (the plan: X [N+1, 6], then U [N, 4 + 2])
    return [(r["u"][i][:4], r["st"][i], r["it"][i], U[i, :, 4:].reshape(-1), r["f"][i], r["resto_iters"][i] + r["resto"][i]) for i in range(len(X))]


def test_optimal_decay_instantiation_against_the_oracle():
    """OptimalDecayMPCCBF with a VTOL2D robot in the multiple-shooting form (the decay rates are two more inputs of a stage, eliminated
    before the recursion -- kernel and oracle take the rows into that Schur complement one at a time, oracle/ms_ipopt.py:_od_eliminate): a
    disc 10 - 30 m ahead of every other aircraft, so that decay rates leave their reference.  Held: same status on every problem; the same
    optimum on >= 97 % of the problems both call optimal (u_0 to 1e-6, decay rates to 1e-5; measured: all, or all but one); iteration counts equal on >= 85 % and within 30 % + 10
    on all (these NLPs are non-convex where a decay rate is active and take 150 - 400 iterations there: the last digits of a long path
    differ); without a disc (odd problems) the solve IS the plain one: iterate for iterate."""
    n = 128
    Xn, up0, gn, on = W.mpc_family_batch("vtol", 4096, 8, seed=0)
    on = on.copy()
    rng = np.random.default_rng(100)
    r = rng.uniform(0.8, 1.6, 4096); d = 10.0 + 20.0 * rng.uniform(size=4096); off = rng.uniform(-1.0, 1.0, 4096)
    on[::2, 0, 0], on[::2, 0, 1], on[::2, 0, 2] = (Xn[:, 0] + d + r)[::2], (Xn[:, 1] + off)[::2], r[::2]
    X, up, goal, obs = Xn[:n], up0[:n], gn[:n], on[:n]
    ctl = sca.BatchedOptimalDecayVtolMSMPCCBF(io_dtype="f64", fallback=False)
    u, rho, st, it = (a.cpu().numpy() for a in ctl.solve(t(X), t(up), t(goal), t(obs)))
    res = oracle_od_many(X, up, goal, obs)
    so = np.array([q[1] for q in res]); ito = np.array([q[2] for q in res])
    assert (st == so).all(), np.flatnonzero(st != so)
    both = (st == 0) & (so == 0)
    assert both.mean() >= 0.9
    du = np.array([np.abs(u[i] - q[0]).max() for i, q in enumerate(res)]); dr = np.array([np.abs(rho[i] - q[3]).max() for i, q in enumerate(res)])
    print(f"od ms: optimal {both.mean():.3f}, iterations equal {np.mean(it == ito):.3f} (mean {ito.mean():.1f} max {ito.max()}), max du {np.sort(du[both])[-3:]} drho {np.sort(dr[both])[-3:]}")
    same = (du <= 1e-6) & (dr <= 1e-5)
    assert same[both].mean() >= 0.97, (np.flatnonzero(both & ~same), du[both].max())       # (a parted one = another local optimum, reached on a 200-iteration path)
    assert np.mean(it[both] == ito[both]) >= 0.85 and (np.abs(it[both] - ito[both]) <= 0.3 * ito[both] + 10).all()
    odd = np.arange(n) % 2 == 1                                           # no disc ahead: decay rates stay at 1, the plain solve
    assert np.abs(rho[odd] - 1.0).max() <= 1e-6 and np.mean(it[odd] == ito[odd]) >= 0.75 and np.abs(it[odd] - ito[odd]).max() <= 3
    moved = np.abs(rho - 1.0).max(axis=1) > 1e-3
    assert moved[~odd].mean() >= 0.5                                      # the discs do move the decay rates
    assert not (st == 4).any()                                            # the restoration phase runs inside the kernel
    # without a workspace the host class hands restorations to the condensed optimal-decay kernel
    raw = sca.BatchedOptimalDecayVtolMSMPCCBF(io_dtype="f64", fallback=False, restoration=False)
    u1, rho1, st1, it1 = raw.solve(t(X), t(up), t(goal), t(obs))
    full = sca.BatchedOptimalDecayVtolMSMPCCBF(io_dtype="f64", restoration=False)
    u2, rho2, st2, it2 = full.solve(t(X), t(up), t(goal), t(obs))
    assert full.n_fallback == int((st1 == 4).sum()) and not bool((st2 == 4).any())
    keep = st1 != 4
    assert torch.equal(u2[keep], u1[keep])


def test_optimal_decay_solves_that_pass_through_the_restoration_phase():
    """The optimal-decay bench batch holds 33 problems (of 4096) on which the regular phase gives up (SC_STATUS_NEEDS_RESTO without a workspace):
    with the restoration phase inside the kernel they are solved there, and the oracle (KERNEL_PROFILE) walks the same way -- measured: 32 of
    33 end with the same status (all optimal but one the stall rule ends in the oracle), 31 with the same input to 1e-6, restoration phases
    of 1 - 100 iterates on both sides (tools/exp_ms_resto_batch.py prints the table).  Held: status equal on >= 90 %, same input on >= 85 %,
    every one of them passes through the restoration in the kernel, none comes back SC_STATUS_NEEDS_RESTO."""
    B = 4096
    Xn, up0, gn, on = W.mpc_family_batch("vtol", B, 8, seed=0)
    on = on.copy()
    rng = np.random.default_rng(100)
    r = rng.uniform(0.8, 1.6, B); d = 10.0 + 20.0 * rng.uniform(size=B); off = rng.uniform(-1.0, 1.0, B)
    on[::2, 0, 0], on[::2, 0, 1], on[::2, 0, 2] = (Xn[:, 0] + d + r)[::2], (Xn[:, 1] + off)[::2], r[::2]
    raw = sca.BatchedOptimalDecayVtolMSMPCCBF(io_dtype="f64", fallback=False, restoration=False)
    st0 = raw.solve(t(Xn), t(up0), t(gn), t(on))[2].cpu().numpy()
    idx = np.flatnonzero(st0 == 4)
    assert 20 <= len(idx) <= 60
    ctl = sca.BatchedOptimalDecayVtolMSMPCCBF(io_dtype="f64", fallback=False)
    u, rho, st, it, tr = (a.cpu().numpy() for a in ctl.solve(t(Xn[idx]), t(up0[idx]), t(gn[idx]), t(on[idx]), want_trace=True))
    res = oracle_od_many(Xn[idx], up0[idx], gn[idx], on[idx])
    so = np.array([q[1] for q in res])
    du = np.array([np.abs(u[k] - q[0]).max() for k, q in enumerate(res)])
    nr = np.array([(tr[k, :it[k] + 1, 7] < 0).sum() for k in range(len(idx))])
    print(f"od restorations: {len(idx)} problems, status equal {int((st == so).sum())}, same input {int((du < 1e-6).sum())}, kernel statuses {np.bincount(st, minlength=3).tolist()}, "
          f"restoration iterates {nr.min()} - {nr.max()}")
    assert not (st == 4).any() and (nr >= 1).all()
    assert np.mean(st == so) >= 0.9 and np.mean(du < 1e-6) >= 0.85 and np.mean(st == 0) >= 0.9


def test_edge_sizes():
    """B = 0 and B = 1; no obstacle at all (K = 0: the solve of a far-away obstacle, to rounding); the largest obstacle count (K = 16), plain and
    optimal decay."""
    X, up, g, ob = W.mpc_family_batch("vtol", 32, 16, seed=1)
    ctl = sca.BatchedVtolMSMPCCBF(io_dtype="f64", fallback=False)
    r0 = ctl.solve(t(X[:0]), t(up[:0]), t(g[:0]), t(ob[:0, :8]))
    assert [tuple(a.shape) for a in r0] == [(0, 4), (0,), (0,)]
    u1, s1, i1 = ctl.solve(t(X[:1]), t(up[:1]), t(g[:1]), t(ob[:1, :8]))
    u8, s8, i8 = ctl.solve(t(X[:8]), t(up[:8]), t(g[:8]), t(ob[:8, :8]))
    assert torch.equal(u1[0], u8[0]) and int(s1[0]) == 0 and int(i1[0]) == int(i8[0])
    none = torch.zeros((32, 0, 7), dtype=torch.float64, device=DEV)
    far = torch.zeros((32, 1, 7), dtype=torch.float64, device=DEV); far[:, 0, 0] = 1e4; far[:, 0, 1] = 1e4; far[:, 0, 2] = 1.0
    ua, sa, ia = ctl.solve(t(X), t(up), t(g), none)
    ub, sb, ib = ctl.solve(t(X), t(up), t(g), far)
    assert bool((sa == 0).all()) and bool((sb == 0).all()) and float((ua - ub).abs().max()) <= 1e-6
    for cls in (sca.BatchedVtolMSMPCCBF, sca.BatchedOptimalDecayVtolMSMPCCBF):
        r = cls(io_dtype="f64", fallback=False).solve(t(X), t(up), t(g), t(ob))
        assert bool((r[-2] == 0).all()) and int(r[-1].max()) < 100


def test_full_bench_batch_is_deterministic_and_position_independent():
    """BASELINE-size batch (4096 aircraft): two launches give the same bits; a problem's result does not depend on its place in the batch (reversed
    order) nor on its neighbours (a slice solved alone); every solve ends optimal and satisfies the NLP it was given -- dynamics residual of the
    returned plan <= 1e-6, CBF rows >= -1e-6 (recomputed on the host from the plan, not read from the solver)."""
    B = 4096
    X, up, g, ob = W.mpc_family_batch("vtol", B, 8, seed=0)
    ctl = sca.BatchedVtolMSMPCCBF(io_dtype="f64", fallback=False)
    u1, s1, i1, p1 = ctl.solve(t(X), t(up), t(g), t(ob), want_plan=True)
    u2, s2, i2, p2 = ctl.solve(t(X), t(up), t(g), t(ob), want_plan=True)
    assert torch.equal(u1, u2) and torch.equal(s1, s2) and torch.equal(i1, i2) and torch.equal(p1, p2)
    ur, sr, ir = ctl.solve(t(X[::-1]), t(up[::-1]), t(g[::-1]), t(ob[::-1]))
    assert torch.equal(ur.flip(0), u1) and torch.equal(ir.flip(0), i1)
    ua, sa, ia = ctl.solve(t(X[1000:1064]), t(up[1000:1064]), t(g[1000:1064]), t(ob[1000:1064]))
    assert torch.equal(ua, u1[1000:1064]) and torch.equal(ia, i1[1000:1064])
    assert bool((s1 == 0).all())
    # the returned plans against the model, on the host (oracle/ms_ipopt.py: the stage functions)
    mdl = MS.vtol_model()
    P = p1.cpu().numpy()
    worst_c, worst_d = 0.0, 0.0
    for i in range(0, B, 97):
        nlp = MS.StageNLP(mdl, X[i], up[i], g[i], ob[i])
        w = np.zeros(nlp.n)
        xs, us = P[i, :31 * 6].reshape(31, 6), P[i, 31 * 6:].reshape(30, 4)
        for k in range(30):
            w[k * 10:k * 10 + 6] = xs[k]; w[k * 10 + 6:(k + 1) * 10] = us[k]
        w[300:] = xs[30]
        ev = nlp.evaluate(w, 0)
        worst_c = max(worst_c, float(np.abs(ev["c"]).max())); worst_d = max(worst_d, float(ev["d"].max()))
    print(f"4096 plans: dynamics residual <= {worst_c:.1e}, CBF rows violated by <= {max(worst_d, 0.0):.1e}")
    assert worst_c <= 1e-6 and worst_d <= 1e-6
