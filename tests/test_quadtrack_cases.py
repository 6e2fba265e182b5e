"""CPU: the injected batches of tests/_quadtrack_cases.py under oracle/tracking_quad.py's select() / apply(u).  Every situation the
GPU test (tests/test_quadtrack_kernels_gpu.py) claims to cover has to be in the batch, no draw may take the oracle outside the
reference's domain, and -- the condition under which the GPU test compares every agent and excuses none -- no comparison the oracle
makes may be closer than 1e-9 to its threshold, unless it is one of the cases built to sit on it exactly."""
import numpy as np
import pytest

import _quadtrack_cases as Q


@pytest.mark.parametrize("model", Q.MODELS)
def test_every_situation_is_in_the_batch(model):
    c = Q.cases(model)
    assert len(c["X"]) == Q.B_MAIN == 200 and Q.B_MAIN % 64 != 0
    tags = Q.tags(model)
    empty = [name for name, mask in tags.items() if not mask.any()]
    assert not empty, f"no agent of the {model} batch is tagged {empty}"
    for name, mask in c["placed"].items():
        assert mask.any(), name
    frozen = c["ret_in"] != 0
    assert 1 / 12 < frozen.mean() < 1 / 6                     # about one in eight
    # in-domain draws only
    idle = c["sm"] == Q.IDLE
    assert (c["wp_index"][idle] == c["n_wp"][idle]).all() and (c["goal"][idle, 3] == 0).all()
    assert (c["wp_index"][~idle] < c["n_wp"][~idle]).all() and (c["wp_index"] >= 0).all()
    assert set(c["n_wp"]) == {1, 2, 3, 4}
    # agents of different kinds share a wave: the four entry states, frozen and running, hit and free in each of the three full waves
    r = Q.reference(model, 0)
    assert r["stepped"][192:].any()                           # the partial wave
    for w in range(3):
        lanes = slice(64 * w, 64 * w + 64)
        assert set(c["sm"][lanes]) == {0, 1, 2, 3} and frozen[lanes].any() and r["hit_before"][lanes].any() and r["stepped"][lanes].any()
    # the obstacle table: circles, superellipsoids of exponent 2, 4 and 2.5, rotated; in the first 7 rows already
    for rows in (c["table"], c["table"][:7]):
        se = np.array([Q.is_superell(o) for o in rows])
        assert (~se).any() and {2.0, 4.0, 2.5} <= set(rows[se, 4]) and (rows[se, 5] != 0).all()
    assert sorted({(f["K"], f["M"]) for f in Q.CONFIGS}) == sorted({(K, M) for K in (1, 8, 9, 16) for M in (0, 1, K - 1, K, 40)})
    assert {f["enable_rotation"] for f in Q.MAIN} == {0, 1} and {f["reached_threshold"] for f in Q.CONFIGS} == {0.3, 0.5}


@pytest.mark.parametrize("model", Q.MODELS)
def test_exact_cases_are_exact(model):
    """The tie agents see the five rows around them at one distance, in the table's order; the exact waypoints are at exactly
    reached_threshold and do not count as reached."""
    c = Q.cases(model)
    r = Q.reference(model, 2)                                 # K = 16, reached_threshold 0.5
    for i in np.flatnonzero(c["placed"]["exact_tie"] & (c["ret_in"] == 0)):
        d = np.hypot(c["table"][list(Q.TIE_ROWS), 0] - c["X"][i, 0], c["table"][list(Q.TIE_ROWS), 1] - c["X"][i, 1])
        assert (d == 1.25).all()
        got = [int(np.flatnonzero((c["table"] == row).all(axis=1))[0]) for row in r["obs_out"][i] if row[0] != 1000.0]
        ties = [m for m in got if m in Q.TIE_ROWS]
        assert ties == sorted(ties) and len(ties) >= 3        # VTOL2D keeps the ones inside its cone
        if model != "VTOL2D":
            assert got[:5] == list(Q.TIE_ROWS)
    ex = np.flatnonzero(c["placed"]["exact_reached"])
    d = np.array([np.linalg.norm(c["X"][i, :2] - c["waypoints"][i, c["wp_index"][i], :2]) for i in ex])
    assert sorted(d) == [0.3] * 3 + [0.5] * 3
    for ci, thr in ((0, 0.3), (2, 0.5)):
        r = Q.reference(model, ci)
        on = ex[d == thr]
        assert (r["margins"]["reached"][on] == 0.0).all() and (r["wp_index"][on] == c["wp_index"][on]).all()
        assert ((r["wp_index"][ex[d < thr]] == c["wp_index"][ex[d < thr]] + 1)).all()


@pytest.mark.parametrize("model", Q.MODELS)
def test_no_draw_raises_and_every_margin_holds(model):
    """Every oracle run the GPU tests use (Q.USED), the f32-rounded ones included: no IndexError / TypeError out of the oracle, and
    every comparison further than 1e-9 from its threshold except the exact cases."""
    seen = set()
    for ci, kind, f32, n in Q.USED:
        r = Q.reference(model, ci, kind, f32, n)
        c = Q.cases(model) if kind == "main" else Q.shared_cases(model)
        bad = Q.margin_violations(c, r, None if n is None else np.arange(n))
        assert not bad, f"{model} configuration {ci} ({kind}, f32={f32}): within {Q.MARGIN} of a threshold: {bad}"
        seen |= set(r["margins"])
        if f32:                                               # the exact distance ties survive the rounding (multiples of 1/4)
            assert (r["order_ties"][c["placed"]["exact_tie"] & (c["ret_in"] == 0)] >= 2).all()
    want = {"reached", "stopped", "rotation", "collision", "order", "wrap"} | ({"cone", "ground", "pitch"} if model == "VTOL2D" else {"clip"})
    assert seen == want
    # shared waypoints: the launch's count is entry 0, the other entries differ from it
    s = Q.shared_cases(model)
    assert s["waypoints"].shape == (Q.W, 3) and s["n_wp"][0] == 3 and (s["n_wp"][1:] != 3).any()
    rs = Q.reference(model, 0, "shared")
    run = s["ret_in"] == 0
    assert (rs["wp_index"][run] > s["wp_index"][run]).any() and (rs["sm"][run] == Q.IDLE).any() and (rs["wp_index"][run] == 2).any()
