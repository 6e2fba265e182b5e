"""CPU: the Gatekeeper / MPS oracle (tests/_shield_oracle.py) against the reference's own run (tests/golden/shield.npz).

Every recorded step of every fixture loop and every single call: the discrete fields (actual_nominal_steps,
current_time_idx, committed length, is_using_backup(), outcome and its step) identical, the floats within 1e-12, and no
recorded decision within 1e-9 of a tie (so the fixtures pin decisions, not rounding)."""
import os

import numpy as np
import pytest

import _shield_oracle as SO
from oracle import backup_cbf as OB

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "shield.npz"))
ALGOS = {"gatekeeper": SO.GATEKEEPER, "mps": SO.MPS}
VARIANTS = ("base", "eo05", "bh2", "nh3", "dt005")


def test_constants_match_the_reference():
    env, spec = OB.default_env(), OB.default_spec()
    assert np.array_equal(G["env"], [env[k] for k in ("hallway_length", "half_width", "pocket_x_min", "pocket_x_max", "pocket_y_min",
                                                      "pocket_y_max", "goal_x_min", "goal_x_max", "bullet_speed", "bullet_length",
                                                      "bullet_width", "bullet_start_x")])
    assert np.array_equal(G["spec"][:4], [spec["radius"], spec["a_max"], spec["v_max"], spec["safety_margin"]])
    assert G["spec"][4] == 5 * 0.1                                        # horizon_discount default 5 dt


@pytest.mark.parametrize("algo", list(ALGOS))
@pytest.mark.parametrize("variant", VARIANTS)
def test_fixture_loop(algo, variant):
    k = f"loop_{algo}_{variant}_"
    dt, bh, nh, eo = G[k + "params"]
    r = SO.closed_loop(ALGOS[algo], dt=dt, backup_horizon=bh, nominal_horizon=nh, event_offset=eo)
    T = len(G[k + "X"])
    assert len(r["X"]) == T
    assert (r["outcome"], r["outcome_step"]) == (int(G[k + "outcome"]), int(G[k + "outcome_step"]))
    for f, g in (("s", "ans"), ("idx", "idx"), ("clen", "clen"), ("using_backup", "using_backup")):
        assert np.array_equal(r[f], G[k + g]), (f, int(np.argmax(r[f] != G[k + g])))
    for f in ("X", "U", "bullet_x", "net"):
        assert np.abs(r[f] - G[k + f]).max() <= 1e-12, f
    assert r["margin"].min() > 1e-9


@pytest.mark.parametrize("algo", list(ALGOS))
def test_fixture_single_calls(algo):
    k = f"calls_{algo}_"
    env, spec = OB.default_env(), OB.default_spec()
    for i in range(len(G[k + "X"])):
        sh = SO.Shield(ALGOS[algo], 0.1, 12.0, 0.05)
        nx, nu = SO.nominal_rollout(G[k + "X"][i], 100, env, spec, 0.1)
        u, info = sh.step(G[k + "X"][i], G[k + "bullet_x"][i], nx, nu)
        assert (info["s"], info["idx"], info["clen"], info["using_backup"]) == (
            G[k + "ans"][i], G[k + "idx"][i], G[k + "clen"][i], G[k + "using_backup"][i]), i
        assert abs(info["net"] - G[k + "net"][i]) <= 1e-12
        assert np.abs(u - G[k + "U"][i]).max() <= 1e-12
        assert info["margin"] > 1e-9
        n = info["clen"]
        assert np.abs(sh.committed_x - G[k + "cx"][i][:n + 1]).max() <= 1e-12
        assert np.abs(sh.committed_u - G[k + "cu"][i][:n]).max() <= 1e-12
        assert np.isnan(G[k + "cx"][i][n + 1:]).all()


# ---- scenario B (tests/_evade_scenarios.py): no two parameters equal, so a wrong field shows --------------------------------
import _evade_scenarios as SC  # noqa: E402

GB = np.load(os.path.join(os.path.dirname(__file__), "golden", "shield_b.npz"))


def test_scenario_b_constants_match_the_reference():
    env, spec = SC.oracle_env(), SC.oracle_spec()
    assert np.array_equal(GB["env"], [env[k] for k in SC.ENV_VECTOR])
    assert np.array_equal(GB["spec"][:4], [spec["radius"], spec["a_max"], spec["v_max"], spec["safety_margin"]])
    assert GB["spec"][4] == 5 * SC.DT["B"]
    assert np.array_equal(GB["gains"], [spec["kp"], spec["kd"]])


@pytest.mark.parametrize("algo", list(ALGOS))
def test_scenario_b_fixture_loop(algo):
    k = f"loop_{algo}_base_"
    dt, bh, nh, eo = GB[k + "params"]
    T = len(GB[k + "X"])
    r = SO.closed_loop(ALGOS[algo], x0=GB[k + "X"][0], bullet_x0=float(GB[k + "bullet_x"][0]), dt=dt, backup_horizon=bh,
                       nominal_horizon=nh, event_offset=eo, tf=(T + 0.5) * dt, env=SC.oracle_env(), spec=SC.oracle_spec())
    assert len(r["X"]) == T
    assert (r["outcome"], r["outcome_step"]) == (int(GB[k + "outcome"]), int(GB[k + "outcome_step"]))
    for f, g in (("s", "ans"), ("idx", "idx"), ("clen", "clen"), ("using_backup", "using_backup")):
        assert np.array_equal(r[f], GB[k + g]), (f, int(np.argmax(r[f] != GB[k + g])))
    for f in ("X", "U", "bullet_x", "net"):
        assert np.abs(r[f] - GB[k + f]).max() <= 1e-12, f
    assert r["margin"].min() > 1e-9
    assert 0 < GB[k + "using_backup"].sum() < T                          # the shield both follows the nominal input and intervenes


@pytest.mark.parametrize("algo", list(ALGOS))
def test_scenario_b_fixture_single_calls(algo):
    k = f"calls_{algo}_"
    dt, bh, nh, eo = GB[f"loop_{algo}_base_params"]
    env, spec = SC.oracle_env(), SC.oracle_spec()
    for i in range(len(GB[k + "X"])):
        sh = SO.Shield(ALGOS[algo], dt, bh, eo, env=env, spec=spec)
        nx, nu = SO.nominal_rollout(GB[k + "X"][i], int(nh / dt), env, spec, dt)
        u, info = sh.step(GB[k + "X"][i], GB[k + "bullet_x"][i], nx, nu)
        assert (info["s"], info["idx"], info["clen"], info["using_backup"]) == (
            GB[k + "ans"][i], GB[k + "idx"][i], GB[k + "clen"][i], GB[k + "using_backup"][i]), i
        assert abs(info["net"] - GB[k + "net"][i]) <= 1e-12
        assert np.abs(u - GB[k + "U"][i]).max() <= 1e-12
        assert info["margin"] > 1e-9
        n = info["clen"]
        assert np.abs(sh.committed_x - GB[k + "cx"][i][:n + 1]).max() <= 1e-12
        assert np.abs(sh.committed_u - GB[k + "cu"][i][:n]).max() <= 1e-12
        assert np.isnan(GB[k + "cx"][i][n + 1:]).all()
