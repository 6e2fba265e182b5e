"""CPU: the float64 oracle of the sensing loop (tests/_unknown_env_oracle.py) against the reference's own runs
(tests/golden/unknown_env.npz, written by tests/golden/make_golden_unknown_env.py from LocalTrackingController.control_step), and
the fleet draws of tests/test_unknown_env_gpu.py through the oracle alone: how many of them come within 1e-6 of deciding a sighting
the other way, which is what that test may exclude."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _unknown_env_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "unknown_env.npz"))


@pytest.mark.parametrize("tag", O.FIXTURE_TAGS)
def test_oracle_reproduces_the_reference_run(fixture, tag):
    z = fixture
    n = len(z[f"{tag}/ret"])
    o = O.oracle_from_fixture(z, tag)
    assert O.SM_INDEX[o.state_machine] == int(z[f"{tag}/sm0"])                 # what set_waypoints left (tracking.py:214-226)
    r = O.run(o, n)
    assert len(r["ret"]) == n
    nx = z[f"{tag}/X"].shape[1]                                                # the single integrator's state is [x, y]
    for k, got in (("X", r["X"][:, :nx]), ("U", r["U"]), ("yaw", r["yaw"])):
        np.testing.assert_allclose(got, z[f"{tag}/{k}"], rtol=1e-9, atol=1e-9, err_msg=k)
    for k in ("sm", "ret", "idx", "mask"):
        assert np.array_equal(r[k], z[f"{tag}/{k}"]), k
    assert np.array_equal(np.isnan(r["u_att"]), np.isnan(z[f"{tag}/u_att"]))    # None at the same steps
    ok = ~np.isnan(r["u_att"])
    np.testing.assert_allclose(r["u_att"][ok], z[f"{tag}/u_att"][ok], rtol=1e-9, atol=1e-9)
    assert o.min_margin > 1e-6 and float(z[f"{tag}/min_margin"]) > 1e-6        # every sighting of the run is decided clearly


def test_fixture_scenes_do_what_they_are_for(fixture):
    z = fixture
    ends = {tag: (len(z[f"{tag}/ret"]), int(z[f"{tag}/ret"][-1])) for tag in O.FIXTURE_TAGS}
    assert ends == {"di_vty": (863, -1), "si_simple": (241, -2), "du": (400, 0), "di_se": (881, -1), "di_forget": (728, -2)}
    first = lambda tag: [int(i) + 1 for i in np.flatnonzero(z[f"{tag}/mask"][1:] != z[f"{tag}/mask"][:-1])]
    assert first("di_vty") == [90, 164, 376, 617] and first("si_simple") == [115] and first("du") == [95, 181]
    assert first("di_se") == [90, 164, 376, 423, 631]
    assert first("di_forget") == [90, 160, 164, 246, 374, 421, 457, 520, 624, 721]                # rows drop out again
    assert int(z["si_simple/mask"][-1]) == 1                                   # it ran into a row it never saw
    for tag in O.FIXTURE_TAGS:                                                 # 'stop' -> 'rotate' -> 'track'
        sm = z[f"{tag}/sm"]
        assert int(z[f"{tag}/sm0"]) == 2 and sm[0] == 3 and (sm == 1).any()


@pytest.mark.parametrize("num_constraints", [10, 5])
def test_fleet_draws_stay_clear_of_the_sighting_thresholds(num_constraints):
    res = O.fleet_oracle(num_constraints)
    assert len(res) == O.FLEET_B == 130
    margins = np.array([float(r["min_margin"]) for r in res])
    print(f"num_constraints {num_constraints}: agents below 1e-6: {int((margins < 1e-6).sum())}, smallest margin {margins.min():.3e}")
    assert (margins < 1e-6).sum() <= 2
    last = np.array([int(r["mask"][-1]) for r in res], dtype=np.uint64)
    assert (last >> np.uint64(32)).astype(bool).any() and (last & np.uint64(0xFFFFFFFF)).astype(bool).any()   # both halves of the mask
    rets = np.array([int(r["ret"][-1]) for r in res])
    assert (rets == 0).any() and (rets == -2).any()
