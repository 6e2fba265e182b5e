"""CPU: oracle/backup_cbf.py (Backup-CBF QP) against tests/golden/backup_cbf.npz -- the reference's own
rollout, finite-difference sensitivities, rows and QP statement executed on its evade scenario
(tests/golden/make_golden_backup.py).  The QP minimiser in the fixture comes from the exact solver (OSQP absent)."""
import os

import numpy as np
import pytest

from oracle import backup_cbf as B

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "backup_cbf.npz"))


def test_environment_and_robot_constants():
    e, s = B.default_env(), B.default_spec()
    assert np.array_equal(G["env"], [e["hallway_length"], e["half_width"], e["pocket_x_min"], e["pocket_x_max"], e["pocket_y_min"],
                                     e["pocket_y_max"], e["goal_x_min"], e["goal_x_max"], e["bullet_speed"], e["bullet_length"],
                                     e["bullet_width"], e["bullet_start_x"]])
    assert np.array_equal(G["spec"], [s["radius"], s["a_max"], s["v_max"], s["safety_margin"], s["alpha"], s["alpha_terminal"]])


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_single_calls_reproduce_the_reference(tag):
    dt, hor = float(G[f"{tag}_dt"]), float(G[f"{tag}_horizon"])
    X, BX = G[f"{tag}_X"], G[f"{tag}_bullet_x"]
    seen = set()
    for i in range(len(X)):
        u, info = B.solve(X[i], G[f"{tag}_u_nom"][i], BX[i], dt, hor, return_info=True)
        n = int(G[f"{tag}_n_rows"][i])
        assert np.abs(info["phi"] - G[f"{tag}_phi"][i]).max() <= 1e-12
        assert np.abs(info["S"] - G[f"{tag}_S"][i]).max() <= 1e-9          # forward differences: 1e-5 / eps amplification
        assert info["n_rows"] == n
        ref = G[f"{tag}_rows"][i][:n]
        assert np.abs(info["rows"] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
        assert info["qp_status"] == int(G[f"{tag}_qp_status"][i])
        assert info["using_backup"] == bool(G[f"{tag}_using_backup"][i])
        assert abs(info["h_min"] - float(G[f"{tag}_h_min"][i])) <= 1e-12
        assert np.abs(u - G[f"{tag}_u"][i]).max() <= 1e-9
        seen.add((info["qp_status"], info["using_backup"]))
    assert len(seen) >= 3                    # solved / infeasible with both fallbacks all occur among the cases


def test_closed_loop_reproduces_the_example():
    T = 260                                  # first bullet pass, the retreat into the pocket and the respawn
    X, U, Bx, UB, HM, outcome, _ = B.closed_loop(G["loop_X"][0], G["loop_bullet_x"][0], T)
    assert outcome == 0 and len(X) == T
    assert np.abs(X - G["loop_X"][:T]).max() <= 1e-8
    assert np.abs(U - G["loop_U"][:T]).max() <= 1e-6
    assert np.array_equal(UB, G["loop_using_backup"][:T])
    assert np.abs(Bx - G["loop_bullet_x"][:T]).max() <= 1e-12
    assert np.abs(HM - G["loop_h_min"][:T]).max() <= 1e-9
    assert X[:, 1].max() > 3.0               # the robot did retreat into the pocket


def test_rows_are_the_definition():
    """A kept row is grad h . S_i . (f0 + g0 u) - grad h . f_pi + dh/dt + alpha h >= 0 (backup_cbf_qp.py:650-661)."""
    i = 3
    x0, bx = G["a_X"][i], float(G["a_bullet_x"][i])
    env, spec = B.default_env(), B.default_spec()
    phi, S = B.rollout(x0, 120, 0.1, env, spec)
    lhs, rhs, keep, _ = B.assemble_rows(x0, phi, S, bx, 0.1, 12.0, env, spec)
    k = 40
    t = k * 0.1
    g = B._fd_grad(lambda z: B.h_safety(z, t, bx, env, spec), phi[k])
    u = np.array([0.3, -0.2])
    xdot = np.array([x0[2], x0[3], u[0], u[1]])
    h = B.h_safety(phi[k], t, bx, env, spec)
    dhdt = (B.h_safety(phi[k], t + 0.1, bx, env, spec) - h) / 0.1
    lhs_def = g @ S[k] @ xdot - g @ ((phi[k + 1] - phi[k]) / 0.1) + dhdt + spec["alpha"] * h
    assert abs((lhs[k - 1] @ u - rhs[k - 1]) - lhs_def) <= 1e-9


# ---- scenario B (tests/_evade_scenarios.py): no two parameters equal, so a wrong field shows --------------------------------
import _evade_scenarios as SC  # noqa: E402

GB = np.load(os.path.join(os.path.dirname(__file__), "golden", "backup_cbf_b.npz"))


def test_scenario_b_constants_and_its_conditions():
    e, s = SC.oracle_env(), SC.oracle_spec()
    assert np.array_equal(GB["env"], [e[k] for k in SC.ENV_VECTOR])
    assert np.array_equal(GB["spec"], [s["radius"], s["a_max"], s["v_max"], s["safety_margin"], s["alpha"], s["alpha_terminal"]])
    assert np.array_equal(GB["gains"], [s["kp"], s["kd"]])
    scalars = [s[k] for k in ("radius", "safety_margin", "a_max", "v_max", "alpha", "alpha_terminal", "kp", "kd")]
    assert len(set(scalars)) == len(scalars)
    assert not set(scalars) & {0.1, 0.2, 1.0, 2.0, 3.0}                  # the literals of the reference's evade code
    kw = SC.ENV_KW["B"]
    assert len({kw["hallway_width"], kw["pocket_width"], kw["bullet_width"]}) == 3
    assert kw["bullet_speed"] != kw["bullet_length"] and 3.0 not in (kw["bullet_speed"], kw["bullet_length"])
    assert kw["goal_length"] != 5 and kw["bullet_start_x"] != -10


def test_scenario_b_single_calls_reproduce_the_reference():
    dt, hor = float(GB["a_dt"]), float(GB["a_horizon"])
    env, spec = SC.oracle_env(), SC.oracle_spec()
    seen = set()
    for i in range(len(GB["a_X"])):
        u, info = B.solve(GB["a_X"][i], GB["a_u_nom"][i], GB["a_bullet_x"][i], dt, hor, env, spec, return_info=True)
        n = int(GB["a_n_rows"][i])
        assert np.abs(info["phi"] - GB["a_phi"][i]).max() <= 1e-12
        assert np.abs(info["S"] - GB["a_S"][i]).max() <= 1e-9
        assert info["n_rows"] == n
        ref = GB["a_rows"][i][:n]
        assert np.abs(info["rows"] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
        assert info["qp_status"] == int(GB["a_qp_status"][i])
        assert info["using_backup"] == bool(GB["a_using_backup"][i])
        assert abs(info["h_min"] - float(GB["a_h_min"][i])) <= 1e-12
        assert np.abs(u - GB["a_u"][i]).max() <= 1e-9
        seen.add((info["qp_status"], info["using_backup"]))
    assert len(seen) == 4                    # solved with and without intervention, infeasible with both fallbacks


@pytest.mark.parametrize("tag,outcome", [("loopg", 1), ("looph", -2), ("loopr", 0)])
def test_scenario_b_closed_loops_reproduce_the_reference(tag, outcome):
    """One loop reaches the goal, one is hit by the bullet, and in one the bullet leaves the hallway and respawns."""
    T = len(GB[f"{tag}_X"])
    X, U, Bx, UB, HM, out, xf = B.closed_loop(GB[f"{tag}_X"][0], GB[f"{tag}_bullet_x"][0], T + 5 if outcome else T, float(GB["a_dt"]),
                                              float(GB["a_horizon"]), SC.oracle_env(), SC.oracle_spec())
    assert out == outcome == int(GB[f"{tag}_outcome"]) and len(X) == T
    assert np.abs(X - GB[f"{tag}_X"]).max() <= 1e-8
    assert np.abs(U - GB[f"{tag}_U"]).max() <= 1e-6
    assert np.array_equal(UB, GB[f"{tag}_using_backup"])
    assert np.abs(Bx - GB[f"{tag}_bullet_x"]).max() <= 1e-12
    assert np.abs(HM - GB[f"{tag}_h_min"]).max() <= 1e-9
    assert np.abs(xf - GB[f"{tag}_final_state"]).max() <= 1e-8
    if tag == "loopr":
        k = int(np.argmax(np.diff(GB[f"{tag}_bullet_x"]) < 0))
        assert GB[f"{tag}_bullet_x"][k + 1] == SC.ENV_KW["B"]["bullet_start_x"] and GB[f"{tag}_bullet_x"][k] > 72.0


def test_confusions_change_the_oracle_on_the_drawn_batch():
    """The power of the scenario-B GPU tests: on their drawn batch, each wrong-field confusion changes what they compare (rows,
    n_rows, h_min, u, status, using_backup, at their tolerances) for at least 10 % of the agents -- for alpha_terminal the
    terminal row alone."""
    X, bx, _ = SC.draw_states_b(SC.BATCH, SC.BATCH_SEED)
    assert np.mean(np.abs(X[:, 0] - SC.oracle_env()["goal_x_min"]) <= 1.5) >= 0.1
    dt, hor = SC.DT["B"], SC.HORIZON["B"]
    ref = SC.solve_many(X, None, bx, dt, hor, SC.oracle_env(), SC.oracle_spec())
    for name, (env, spec) in SC.confusions().items():
        got = SC.solve_many(X, None, bx, dt, hor, env, spec)
        if name.startswith("alpha_terminal"):                             # only the terminal row (the last kept one) counts
            n = ref["n_rows"]
            assert np.array_equal(got["n_rows"], n)
            last = lambda r: np.array([r["rows"][i][n[i] - 1] if n[i] else np.zeros(3) for i in range(len(n))])
            scale = np.array([max(1.0, np.abs(ref["rows"][i][:n[i]]).max()) if n[i] else 1.0 for i in range(len(n))])
            differs = np.abs(last(got) - last(ref)).max(axis=1) > SC.ROW_TOL * scale
        else:
            differs = SC.compare(got, ref)[1]
        print(f"{name:32s} changes {100 * differs.mean():5.1f} % of {len(X)} agents")
        assert differs.mean() >= 0.1, name
