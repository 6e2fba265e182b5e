"""GPU: kernel 13 (csrc/mpc_du_ms.hip) instantiated for Unicycle2D -- the reference's MPC-CBF NLP for that robot as do-mpc poses it
(position_control/mpc_cbf.py:22-24,52-53,135-141,188-192,312-315; robots/unicycle2D.py:42-68,127-146: three states, inputs (v, omega), ONE-step
rows d_h + alpha h_k >= 0) under IPOPT's algorithm -- against oracle/ms_ipopt.py with uni_model() in the kernel's profile: same status, same
iteration count, |u0 - u0_oracle| <= 1e-8.  The kernel holds the robot as four states, the last one idle."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import safe_control_amd as sca  # noqa: E402
from safe_control_amd import workloads as W  # noqa: E402
from safe_control_amd.robots.spec import complete_robot_spec  # noqa: E402
from oracle import ms_ipopt as MS  # noqa: E402
from _oracle_pool import ms_batch, ms_solve_many, take  # noqa: E402

DEV = "cuda:0"
SPEC = {"model": "Unicycle2D"}


def t(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def uni_oracle_model():
    sp = complete_robot_spec(dict(SPEC))
    return MS.uni_model({k: v for k, v in sp.items() if k in MS.uni_model()["spec"]})


def oracle_many(X, up, goal, obs, N=None):
    """oracle/ms_ipopt.py (kernel 13's profile) on every row, in the host's child-process pool (tests/_oracle_pool.py)."""
    return ms_solve_many("uni", X, up, goal, obs, opts=dict(MS.KERNEL13_PROFILE), N=N, spec=SPEC)


def compare(u, st, it, res, n_off):
    so, ito = res["st"], res["it"]
    assert np.array_equal(st, so), np.flatnonzero(st != so)[:10]
    off = it != ito
    assert off.sum() <= n_off and np.abs(it - ito).max() <= 2, (int(off.sum()), int(np.abs(it - ito).max()))
    du = np.abs(u - res["u"]).max(axis=1)
    assert du[~off].max() <= 1e-8 and du.max() <= 1e-6, (du[~off].max(), du.max())
    return so, ito


def test_bench_draws_and_a_crowded_scene_against_the_oracle():
    n = 256
    (X, up, goal, obs), res = ms_batch("uni", 0, opts=dict(MS.KERNEL13_PROFILE), spec=SPEC)     # (the session's run over all 4096: tests/test_mpccbf_ms_full_batch_gpu.py)
    X, up, goal, obs, res = X[:n].copy(), up[:n].copy(), goal[:n].copy(), obs[:n].copy(), take(res, slice(0, n))
    ctl = sca.BatchedMSMPCCBF(SPEC, io_dtype="f64")
    u, st, it, plan = (a.cpu().numpy() for a in ctl.solve(t(X), t(up), t(goal), t(obs), want_plan=True))
    so, ito = compare(u, st, it, res, n_off=4)
    # the plan: states as four columns (the idle one stays zero), the oracle's as three
    P4 = plan[:, : 11 * 4].reshape(n, 11, 4)
    assert np.abs(P4[:, :, 3]).max() == 0.0
    Po = res["plan"][:, : 11 * 3].reshape(n, 11, 3)
    assert np.abs(P4[:, :, :3] - Po)[so == 0].max() <= 1e-6
    # obstacles pulled to within 0.6 m of the robot and a last input at full speed: rows active or violated at the start
    rng = np.random.default_rng(7)
    m = 128
    ob2 = obs[:m].copy()
    ang = rng.uniform(0, 2 * np.pi, (m, 3)); rad = rng.uniform(0.45, 0.9, (m, 3))
    ob2[:, :3, 0] = X[:m, None, 0] + rad * np.cos(ang); ob2[:, :3, 1] = X[:m, None, 1] + rad * np.sin(ang); ob2[:, :3, 2] = 0.2
    up2 = np.column_stack([rng.uniform(0.5, 1.0, m), rng.uniform(-0.5, 0.5, m)])
    u, st, it = (a.cpu().numpy() for a in ctl.solve(t(X[:m]), t(up2), t(goal[:m]), t(ob2)))
    s2, i2 = compare(u, st, it, oracle_many(X[:m], up2, goal[:m], ob2), n_off=4)
    print(f"uni ms kernel: bench draws optimal {np.mean(so == 0):.4f}, iterations mean {ito.mean():.1f} max {ito.max()}; crowded: optimal {np.mean(s2 == 0):.4f} "
          f"infeasible {np.mean(s2 == 1):.4f}, iterations max {i2.max()}")


def test_full_batch_f32_storage_and_the_condensed_kernel():
    X, up, goal, obs = W.mpc_family_batch("uni", 4096, 8, seed=0)
    f = lambda a: t(a.astype(np.float32), torch.float32)                          # noqa: E731
    ctl = sca.BatchedMSMPCCBF(SPEC, io_dtype="f32")
    u1, s1, i1 = ctl.solve(f(X), f(up), f(goal), f(obs))
    u2, s2, i2 = ctl.solve(f(X), f(up), f(goal), f(obs))
    assert torch.equal(u1, u2) and torch.equal(s1, s2) and torch.equal(i1, i2)
    assert (u1[:, 0].abs() <= 1.0 + 1e-6).all() and (u1[:, 1].abs() <= 0.5 + 1e-6).all()
    uc, sc, ic = sca.BatchedMPCCBF(SPEC, io_dtype="f32").solve(f(X), f(up), f(goal), f(obs))[:3]
    both = (s1 == 0) & (sc == 0)
    same = ((u1 - uc).abs().amax(dim=1) <= 1e-4)[both].double().mean().item()
    assert both.double().mean().item() >= 0.97 and same >= 0.99, (both.double().mean().item(), same)
    print(f"uni ms kernel, 4096: optimal {(s1 == 0).double().mean().item():.4f}, iterations mean {i1.double().mean().item():.1f} max {int(i1.max())}; same optimum as the condensed kernel on {same:.4f}")


def test_drop_in_class_and_batched_loop_use_the_kernel():
    from safe_control_amd.position_control.mpc_cbf import MPCCBF

    class Robot:
        dt, robot_radius = 0.05, 0.25
    assert MPCCBF(Robot(), {"model": "Unicycle2D", "mpc_formulation": "condensed"}, num_obs=8)._ms is None
    ctl = MPCCBF(Robot(), {"model": "Unicycle2D"}, num_obs=8)
    assert ctl._ms is not None
    X, up, goal, obs = (a[:2] for a in W.mpc_family_batch("uni", 64, 8, seed=2))
    u = ctl.solve_control_problem(X[0, :3].reshape(-1, 1), dict(goal=goal[0], state_machine="track", u_ref=np.zeros((2, 1))), obs[0])
    uo = MS.solve(uni_oracle_model(), X[0], np.zeros(2), goal[0], obs[0], opts=dict(MS.KERNEL_PROFILE))[0]
    assert np.abs(u.reshape(-1) - uo).max() <= 1e-8
    loop = sca.BatchedTrackingController(X[:, :3], {"model": "Unicycle2D"}, controller_type={"pos": "mpc_cbf"}, obs=obs[0], device=DEV)
    assert loop.mpc_ms is not None and loop.mpc_ms.model == "Unicycle2D"
