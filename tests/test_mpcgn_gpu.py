"""GPU: MPC-CBF kernel for DoubleIntegrator2D / Quad2D (csrc/mpc_gn.hip) through the C-ABI against the
numpy oracle (oracle/mpc_gn.py problem functions with a Gauss-Newton Hessian + oracle/mpc_cbf.py solver).  The kernel
follows the oracle's interior-point method iterate for iterate: same status, iteration counts within 2,
|u0 - u0_oracle| <= 1e-6, |z - z_oracle| <= 2e-5 (looser only where the oracle itself stopped on the acceptable-point rule)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import safe_control_amd as sca  # noqa: E402
from oracle import mpc_cbf as M  # noqa: E402
from oracle import mpc_gn as G  # noqa: E402

DEV = "cuda:0"
MODELS = {"DoubleIntegrator2D": G.di_model, "Quad2D": G.quad2d_model}


def t(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def draw(mdl, rng, K):
    nx = mdl["nx"]
    x0 = np.zeros(nx); x0[:2] = rng.uniform(0, 14, 2)
    if mdl["name"] == "KinematicBicycle2D":
        x0[2] = rng.uniform(-np.pi, np.pi); x0[3] = rng.uniform(0.2, 2.0)
    elif mdl["name"] == "DoubleIntegrator2D":
        x0[2:4] = rng.uniform(-0.75, 0.75, 2)                      # some above v_max = 1 in norm after a step: rescaling active
    else:
        x0[2] = rng.uniform(-0.2, 0.2); x0[3:5] = rng.uniform(-0.5, 0.5, 2)
    goal = rng.uniform(0, 14, 2)
    obs = np.tile(M.DUMMY_OBS, (K, 1))
    for j in range(max(1, K - 1)):
        r = rng.uniform(0.2, 1.0); rho = rng.uniform(r + mdl["radius"] + 0.3, 4.0); ph = rng.uniform(-np.pi, np.pi)
        obs[j] = [x0[0] + rho * np.cos(ph), x0[1] + rho * np.sin(ph), r, 0, 0, 0, 0]
    return x0, goal, obs


def u_start(mdl):
    return (mdl["u_lo"] + mdl["u_hi"]) / 2 if mdl["name"] == "Quad2D" else np.zeros(2)


@pytest.mark.parametrize("name,N,K", [("DoubleIntegrator2D", 10, 8), ("Quad2D", 10, 8), ("DoubleIntegrator2D", 14, 4), ("Quad2D", 5, 2)])
def test_batch_matches_oracle(name, N, K):
    B = 20
    mdl = MODELS[name]()
    rng = np.random.default_rng(N * 10 + K)
    X = np.zeros((B, mdl["nx"])); Gl = np.zeros((B, 2)); O = np.zeros((B, K, 7))
    for i in range(B):
        X[i], Gl[i], O[i] = draw(mdl, rng, K)
    up = np.tile(u_start(mdl), (B, 1))
    ctl = sca.BatchedGnMPCCBF({"model": name}, io_dtype="f64", horizon=N)
    u, st, it, z = ctl.solve(t(X), t(up), t(Gl), t(O), want_z=True)
    torch.cuda.synchronize()
    u, st, it, z = u.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy(), z.cpu().numpy()
    n_opt = n_act = 0
    for i in range(B):
        uo, so, ito, info = G.solve(mdl, X[i], up[i], Gl[i], O[i], N=N, return_info=True)
        assert st[i] == so, f"status differs at problem {i}: {st[i]} vs {so}"          # the bar of tests/test_mpccbf_gpu.py
        if so == 0:
            # (an optimum that stopped on the acceptable rule: both solvers are then within acceptable_tol of the same point)
            tol_u, tol_z = (1e-6, 2e-5) if info["err"] <= 1e-6 else (1e-4, 1e-3)
            assert np.abs(u[i] - uo).max() <= tol_u * max(1.0, np.abs(uo).max()), i
            assert np.abs(z[i] - info["z"]).max() <= tol_z * max(1.0, np.abs(info["z"]).max()), i
            assert abs(int(it[i]) - ito) <= 2, i
            n_opt += 1
            n_act += int(np.min(info["g"][: N * K]) < 1e-4)
        elif so == 1:
            assert info["theta"] > 1e-6 and np.abs(u[i] - uo).max() <= 1e-5 * max(1.0, np.abs(uo).max()), i
    assert n_opt >= B // 2 and (n_act >= 1 or N < 10)


def test_double_integrator_superellipsoid_f32_and_shared_table():
    B, K, N = 16, 3, 10
    mdl = G.di_model()
    rng = np.random.default_rng(4)
    X = np.zeros((B, 4)); Gl = np.zeros((B, 2)); O = np.zeros((B, K, 7))
    for i in range(B):
        X[i], Gl[i], O[i] = draw(mdl, rng, K)
        rho, ph = rng.uniform(1.8, 3.0), rng.uniform(-np.pi, np.pi)
        O[i, 1] = [X[i, 0] + rho * np.cos(ph), X[i, 1] + rho * np.sin(ph), *rng.uniform(0.4, 1.0, 2), float(rng.choice([2, 4, 6])),
                   rng.uniform(-3, 3), 1.0]
    ctl = sca.BatchedGnMPCCBF({"model": "DoubleIntegrator2D"}, io_dtype="f64", horizon=N)
    u, st, it = ctl.solve(t(X), t(np.zeros((B, 2))), t(Gl), t(O))
    u, st = u.cpu().numpy(), st.cpu().numpy()
    for i in range(B):
        uo, so, _, info = G.solve(mdl, X[i], np.zeros(2), Gl[i], O[i], N=N, return_info=True)
        assert st[i] == so
        if so == 0:
            assert np.abs(u[i] - uo).max() <= (1e-6 if info["err"] <= 1e-6 else 1e-4)
    # f32 arrays, one shared table
    shared = O[0].copy(); shared[:, :2] += 40.0
    X32, G32, S32 = X.astype(np.float32), Gl.astype(np.float32), shared.astype(np.float32)
    ctl32 = sca.BatchedGnMPCCBF({"model": "DoubleIntegrator2D"}, io_dtype="f32", horizon=N)
    u, st, it = ctl32.solve(t(X32, torch.float32), t(np.zeros((B, 2)), torch.float32), t(G32, torch.float32), t(S32, torch.float32))
    u, st = u.double().cpu().numpy(), st.cpu().numpy()
    for i in range(0, B, 3):
        uo, so, _, info = G.solve(mdl, X32[i].astype(np.float64), np.zeros(2), G32[i].astype(np.float64), S32.astype(np.float64),
                                  N=N, return_info=True)
        assert st[i] == so
        if so == 0:
            assert np.abs(u[i] - uo).max() <= (2e-6 if info["err"] <= 1e-6 else 1e-4) * max(1.0, np.abs(uo).max())


def test_drop_in_class_and_bad_arguments():
    for name in MODELS:
        mdl = MODELS[name]()
        rng = np.random.default_rng(8)
        x0, goal, obs = draw(mdl, rng, 3)
        robot = sca.RobotHandle(x0, {"model": name})
        ctl = sca.MPCCBF(robot, robot.robot_spec, num_obs=5)
        assert type(ctl).__name__ == "GnMPCCBF" and ctl.horizon == 10 and ctl.status == "optimal"
        ctl.u_prev = u_start(mdl).copy()
        ref = {"state_machine": "track", "u_ref": np.zeros((2, 1)), "goal": goal}
        u = ctl.solve_control_problem(robot.X, ref, obs[:2, :3])
        uo, so, _, info = G.solve(mdl, x0, u_start(mdl), goal, M.pad_obstacles(obs[:2, :3], 5), return_info=True)
        if so == 0:
            assert ctl.solver_status == "optimal" and u.shape == (2, 1)
            assert np.abs(u.reshape(-1) - uo).max() <= (1e-6 if info["err"] <= 1e-6 else 1e-4) * max(1.0, np.abs(uo).max())
        ref["state_machine"] = "stop"
        assert ctl.solve_control_problem(robot.X, ref, None) is ref["u_ref"]
    with pytest.raises(NotImplementedError):
        sca.BatchedGnMPCCBF({"model": "Unicycle2D"})                   # rel-degree-1 distance barrier: csrc/mpc_cbf.hip serves it
    ctl = sca.BatchedGnMPCCBF({"model": "Quad2D"})
    with pytest.raises(ValueError):
        ctl.solve(t(np.zeros((2, 4))), t(np.zeros((2, 2))), t(np.zeros((2, 2))), t(np.zeros((2, 1, 7))))


def test_drop_in_double_integrator_on_this_kernel():
    """robot_spec['mpc_formulation'] = 'condensed': the DoubleIntegrator2D drop-in on this kernel's host-pointer entry point (its default is
    kernel 13, which the loop above runs).  Two agents, one obstacle, horizon 5."""
    mdl = G.di_model()
    rng = np.random.default_rng(5)
    for _ in range(2):
        x0, goal, obs = draw(mdl, rng, 1)
        robot = sca.RobotHandle(x0, {"model": "DoubleIntegrator2D"})
        ctl = sca.MPCCBF(robot, dict(robot.robot_spec, mpc_formulation="condensed", mpc_horizon=5), num_obs=1)
        assert type(ctl).__name__ == "GnMPCCBF" and ctl._ms is None and ctl.horizon == 5
        u = ctl.solve_control_problem(robot.X, {"state_machine": "track", "u_ref": np.zeros((2, 1)), "goal": goal}, obs)
        uo, so, _, info = G.solve(mdl, x0, np.zeros(2), goal, obs, N=5, return_info=True)
        assert ctl.solver_status == sca._lib.STATUS_STRINGS[so]
        if so == 0:
            assert u.shape == (2, 1) and np.abs(u.reshape(-1) - uo).max() <= (1e-6 if info["err"] <= 1e-6 else 1e-4) * max(1.0, np.abs(uo).max())


def test_non_finite_inputs_terminate_and_are_not_reported_optimal():
    for name in MODELS:
        mdl = MODELS[name]()
        rng = np.random.default_rng(1)
        X = np.zeros((4, mdl["nx"])); Gl = np.zeros((4, 2)); O = np.zeros((4, 3, 7))
        for i in range(4):
            X[i], Gl[i], O[i] = draw(mdl, rng, 3)
        X[1, 0] = np.nan; Gl[2, 1] = np.inf; O[3, 0, 2] = np.nan
        ctl = sca.BatchedGnMPCCBF({"model": name}, io_dtype="f64", horizon=10)
        u, st, it = ctl.solve(t(X), t(np.tile(u_start(mdl), (4, 1))), t(Gl), t(O))
        torch.cuda.synchronize()
        st = st.cpu().numpy()
        assert np.all(st[1:] != 0) and np.all(it.cpu().numpy() <= 3000)


@pytest.mark.parametrize("name", ["DoubleIntegrator2D", "Quad2D"])
def test_full_batch_properties(name):
    """4096 problems: deterministic launches, termination within the iteration limit, reported optima feasible (oracle's
    constraint functions on a strided sample) and inside the input box."""
    B, K, N = 4096, 8, 10
    mdl = MODELS[name]()
    rng = np.random.default_rng(21)
    X = np.zeros((B, mdl["nx"])); Gl = np.zeros((B, 2)); O = np.zeros((B, K, 7))
    for i in range(B):
        X[i], Gl[i], O[i] = draw(mdl, rng, K)
    up = np.tile(u_start(mdl), (B, 1))
    ctl = sca.BatchedGnMPCCBF({"model": name}, io_dtype="f64", horizon=N)
    args = (t(X), t(up), t(Gl), t(O))
    u1, s1, i1, z1 = ctl.solve(*args, want_z=True)
    u2, s2, i2, z2 = ctl.solve(*args, want_z=True)
    torch.cuda.synchronize()
    assert torch.equal(u1, u2) and torch.equal(s1, s2) and torch.equal(i1, i2) and torch.equal(z1, z2)
    st, it, z = s1.cpu().numpy(), i1.cpu().numpy(), z1.cpu().numpy()
    assert it.max() <= 3000 and set(np.unique(st)) <= {0, 1, 2} and (st == 0).mean() > 0.85
    lo, hi = np.tile(mdl["u_lo"], N), np.tile(mdl["u_hi"], N)
    ok = st == 0
    assert np.all(z[ok] >= lo - 1e-9) and np.all(z[ok] <= hi + 1e-9)
    P = G.params(mdl, N)
    for i in np.flatnonzero(ok)[::97]:
        g = G.evaluate(X[i], z[i], up[i], Gl[i], O[i], P, level=0)["g"]
        assert g.min() >= -1e-6
