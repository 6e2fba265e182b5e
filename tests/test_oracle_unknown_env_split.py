"""CPU: the split oracle of the sensing loop (tests/_unknown_env_split_oracle.py) with the parent's own CBF-QP behind ``solve_fn``
IS the parent oracle on the five scenes of tests/golden/unknown_env.npz -- X, U, yaw, u_att, state machine, return codes and masks
exactly equal -- so its control flow is the pinned one; and the fleet draws of tests/test_unknown_env_split_gpu.py through the
split oracle alone: how many come within 1e-6 of deciding a sighting the other way, which is what that test may exclude."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _unknown_env_oracle as O  # noqa: E402
import _unknown_env_split_oracle as S  # noqa: E402


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "unknown_env.npz"))


def split_from_fixture(z, tag):
    mi = int(z[f"{tag}/model"])
    X, yaw = O.state_and_yaw(mi, z[f"{tag}/x0"])
    o = S.UnknownEnvSplitOracle(O.MODELS[mi], X, O.fixture_spec(z, tag), obs=z[f"{tag}/obs"], unknown_obs=z[f"{tag}/unknown"],
                                att=O.ATTS[int(z[f"{tag}/att"])] or "velocity_tracking_yaw", yaw0=yaw, solve_fn=lambda *a: None)
    o.split_solve_fn = S.cbf_qp_solve_fn(o)
    o.set_waypoints(z[f"{tag}/waypoints"])
    return o


@pytest.mark.parametrize("tag", O.FIXTURE_TAGS)
def test_split_oracle_is_the_parent_with_its_own_solver(fixture, tag):
    z = fixture
    n = len(z[f"{tag}/ret"])
    parent = O.run(O.oracle_from_fixture(z, tag), n)
    o = split_from_fixture(z, tag)
    assert O.SM_INDEX[o.state_machine] == int(z[f"{tag}/sm0"])
    # the parent ends a run whose QP has no solution with -2 and the split loop has no such exit: cbf_qp_solve_fn raises there.  None
    # of the five scenes ends that way (the two that end with -2 collide).
    got = O.run(o, n)
    assert len(got["ret"]) == len(parent["ret"]) == n
    for k in ("X", "U", "yaw", "sm", "ret", "idx", "mask"):
        assert np.array_equal(got[k], parent[k]), k
    assert np.array_equal(got["u_att"], parent["u_att"], equal_nan=True)
    assert o.min_margin > 1e-6


def test_split_oracle_needs_a_solver_and_never_reports_failure():
    with pytest.raises(ValueError):
        S.UnknownEnvSplitOracle(O.MODELS[2], np.zeros(4), dict(O.FLEET_SPEC))
    # a solver that returns (u, status) with a failing status is still 'optimal' to the loop (mpc_cbf.py:10)
    o = S.UnknownEnvSplitOracle(O.MODELS[2], np.array([2.0, 2.0, 0.0, 0.0]), dict(O.FLEET_SPEC), yaw0=0.0,
                                solve_fn=lambda X, cref, nobs: (np.array([0.1, 0.0]), 5))
    o.set_waypoints(np.array([[6.0, 2.0]]))
    assert o.control_step() == 0 and o.status == 0 and np.array_equal(o.u_pos, [0.1, 0.0])


@pytest.mark.parametrize("num_constraints", [10, 5])
def test_fleet_draws_of_the_split_loop_stay_clear_of_the_sighting_thresholds(num_constraints):
    res = S.fleet_split_oracle(num_constraints)
    assert len(res) == O.FLEET_B == 130
    margins = np.array([float(r["min_margin"]) for r in res])
    print(f"num_constraints {num_constraints}: agents below 1e-6: {int((margins < 1e-6).sum())}, smallest margin {margins.min():.3e}")
    assert (margins < 1e-6).sum() <= 2
    last = np.array([int(r["mask"][-1]) for r in res], dtype=np.uint64)
    assert (last >> np.uint64(32)).astype(bool).any() and (last & np.uint64(0xFFFFFFFF)).astype(bool).any()   # both halves of the mask
    assert all(len(r["ret"]) >= 1 for r in res)
