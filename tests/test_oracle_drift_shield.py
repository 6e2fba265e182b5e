"""The numpy oracle of the drift-car shields (tests/_drift_shield_oracle.py) against the reference's own run
(tests/golden/drift_shield.npz, written by tests/golden/make_golden_drift_shield.py).

Teacher-forced: each step of each of the 16 loops is one call from the fixture's recorded state, friction and obstacle
positions, with the shield state carried along.  Decisions (s, index, committed length, using-backup) must be equal on every
step whose decision margin is at least 1e-9 m, the inputs equal to a relative 1e-9 (numpy against numpy: equal to the last bit
where the libm is the same).  Free-running, the oracle reproduces outcome and outcome step of every loop the fixture marks
stable (a second reference run from a start moved by 1e-12 took the same decisions)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _drift_shield_oracle as O  # noqa: E402

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drift_shield.npz"))
ALGOS = {"gatekeeper": O.GATEKEEPER, "mps": O.MPS}
BACKUPS = {"lane_change": O.LANE_CHANGE, "stop": O.STOP}
CASES = ("high_friction", "middle_lane_only", "low_friction", "puddle_surprise")
LOOPS = [(a, b, c) for a in ALGOS for b in BACKUPS for c in CASES]
TAU_DOT_MAX = 8000.0


def loop(a, b, c):
    pre = f"loop_{a}_{b}_{c}_"
    return {k[len(pre):]: G[k] for k in G.files if k.startswith(pre)}


def ctrl(b, sp=None):
    sp = sp or O.default_spec()
    return O.stop_ctrl(sp) if BACKUPS[b] == O.STOP else O.lane_change_ctrl(sp, O.lane_center(O.default_track(), 3))


def table(L, k):
    m = L["mobs0"].copy()
    m[:, :2] = L["mobs"][k]
    return m


def input_error(u, ref):
    return max(abs(u[0] - ref[0]), abs(u[1] - ref[1]) / TAU_DOT_MAX)


@pytest.mark.parametrize("a,b,c", LOOPS)
def test_teacher_forced(a, b, c):
    L = loop(a, b, c)
    sp = dict(O.default_spec(), mu=float(L["mu0"]))
    sh = O.Shield(ALGOS[a], ctrl(b, sp), O.default_track(), sp)
    worst, left_out = 0.0, 0
    for k in range(len(L["U"])):
        nx, nu = O.nominal_rollout(L["X"][k], 120, O.default_track(), float(L["friction"][k]), sp, 0.05)
        u, info = sh.step(L["X"][k], float(L["friction"][k]), nx, nu, (), table(L, k))
        if info["margin"] < 1e-9:
            left_out += 1
            pytest.fail(f"step {k}: margin {info['margin']:.3g} below 1e-9 in the reference's own loop")
        got = (info["s"], info["idx"], info["clen"], info["using_backup"], info["net"])
        want = (int(L["ans"][k]), int(L["idx"][k]), int(L["clen"][k]), bool(L["using_backup"][k]), float(L["net"][k]))
        assert got == want, f"step {k}: {got} != {want}"
        worst = max(worst, input_error(u, L["U"][k]))
    print(f"{a} {b} {c}: {len(L['U'])} steps, worst input error {worst:.3g}, left out {left_out}")
    assert worst <= 1e-9


def test_single_calls():
    n = len(G["calls_U"])
    assert n >= 24
    n_static, n_moving = (~np.isnan(G["calls_sobs"][:, :, 0])).sum(axis=1), (~np.isnan(G["calls_mobs"][:, :, 0])).sum(axis=1)
    assert {0, 1, 2} <= set(n_static.tolist()) and {1, 2, 8} <= set(n_moving.tolist())      # static circles; 1, 2 and 8 moving rows
    for i in range(n):
        b = ("lane_change", "stop")[int(G["calls_backup"][i])]
        mu = float(G["calls_friction"][i])
        sp = dict(O.default_spec(), mu=mu)
        sh = O.Shield(int(G["calls_algo"][i]), ctrl(b, sp), O.default_track(), sp)
        mobs = G["calls_mobs"][i]
        mobs = mobs[~np.isnan(mobs[:, 0])]
        sobs = G["calls_sobs"][i]
        sobs = sobs[~np.isnan(sobs[:, 0])]
        nx, nu = G["calls_nx"][i], G["calls_nu"][i]
        rx, ru = O.nominal_rollout(G["calls_X"][i], 120, O.default_track(), mu, sp, 0.05)
        assert np.array_equal(rx, nx) and np.array_equal(ru, nu), "the oracle's lane keeper is the fixture's"
        u, info = sh.step(G["calls_X"][i], mu, nx, nu, sobs, mobs)
        assert info["margin"] >= 1e-9
        assert (info["s"], info["idx"], info["clen"], info["using_backup"]) == (
            int(G["calls_ans"][i]), int(G["calls_idx"][i]), int(G["calls_clen"][i]), bool(G["calls_using_backup"][i]))
        assert input_error(u, G["calls_U"][i]) <= 1e-9
        s = info["s"]
        cb = G["calls_cb"][i]
        assert np.abs(sh.committed_x[s:] - cb[:, :8]).max() <= 1e-9 * 300 and np.allclose(sh.committed_u[s:], cb[:-1, 8:], rtol=1e-9, atol=1e-9)


STABLE = [l for l in LOOPS if bool(G["loop_%s_%s_%s_stable" % l])]    # the others sit on a tie in the reference itself: teacher-forced only


def test_the_fixture_knows_which_loops_sit_on_a_tie():
    assert sorted(set(LOOPS) - set(STABLE)) == [("gatekeeper", "stop", "high_friction"), ("mps", "stop", "high_friction")]


@pytest.mark.parametrize("a,b,c", STABLE)
def test_free_run(a, b, c):
    L = loop(a, b, c)
    out = O.closed_loop(ALGOS[a], ctrl(b, dict(O.default_spec(), mu=float(L["mu0"]))), L["X"][0], L["mobs0"], puddles=L["puddles"],
                        mu0=float(L["mu0"]))
    assert (out["outcome"], out["outcome_step"]) == (int(L["outcome"]), int(L["outcome_step"]))
    assert out["backup_steps"] == int(L["using_backup"].sum())
