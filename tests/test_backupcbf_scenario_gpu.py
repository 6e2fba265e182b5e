"""GPU: the Backup-CBF QP kernel (csrc/backup_cbf.hip) at scenario B of tests/_evade_scenarios.py -- no two scenario parameters
equal and none equal to a literal of the reference's evade code, so a kernel or a host layer (make_params, the parameter
fill of BatchedBackupCBF) that reads the wrong field fails here; tests/test_oracle_backup.py shows that every such confusion
changes the oracle for at least a tenth of the drawn batch.  Everything runs through BatchedBackupCBF and is held to
oracle/backup_cbf.py, which tests/golden/backup_cbf_b.npz pins on the reference's own run at this scenario.

Tolerances are those of tests/test_backupcbf_gpu.py for float64 storage (tests/_evade_scenarios.compare): kept rows
1e-7 max(1, |row|_inf), u 1e-6, h_min 1e-9, n_rows / status / using_backup equal.  An agent whose status or row count
disagrees may be set aside only if the oracle's QP is within 1e-6 of flipping (oracle.qp.feasibility_margin) or a row's |lhs|
is within 1e-9 of the keep threshold, and at most 1 % of a batch; the oracle runs are shared between the tests.

Status -1 (no row kept) cannot be reached inside the map at N = 90: row 1 has |lhs| = dt |grad h|, and grad h is a unit vector
unless the agent sits inside the bullet's box, which it cannot for a whole horizon.  The drawn batch therefore ends with four
agents 1e12 m outside the map, where x + 1e-5 == x and every forward difference of h is exactly zero."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _evade_scenarios as SC  # noqa: E402
import safe_control_amd as sca  # noqa: E402
from safe_control_amd import _lib  # noqa: E402
from safe_control_amd.position_control import backup_cbf_qp as BK  # noqa: E402

DEV = "cuda:0"
GB = np.load(os.path.join(os.path.dirname(__file__), "golden", "backup_cbf_b.npz"))
DT, HOR = SC.DT["B"], SC.HORIZON["B"]
F32 = 2.0 ** -23
SENTINEL = -77


def t(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def controller(horizon=HOR, io_dtype="f64"):
    ctl = sca.BatchedBackupCBF(robot_spec=SC.ROBOT["B"], env=SC.kernel_env("B"), dt=DT, backup_horizon=horizon, io_dtype=io_dtype)
    ctl.alpha, ctl.alpha_terminal = SC.CBF["B"]["alpha"], SC.CBF["B"]["alpha_terminal"]
    ctl.kp, ctl.kd = SC.GAINS["B"]["kp"], SC.GAINS["B"]["kd"]
    return ctl


def solve(ctl, X, u_nom, bx, out=None):
    dt_ = ctl.torch_dtype
    r = ctl.solve(t(X, dt_), None if u_nom is None else t(u_nom, dt_), t(np.atleast_1d(bx), dt_), want_rows=True, out=out)
    torch.cuda.synchronize()
    u, st, using, hmin, n_rows, rows = (a.double().cpu().numpy() if a.is_floating_point() else a.cpu().numpy() for a in r)
    return dict(u=u, status=st, using_backup=using, h_min=hmin, n_rows=n_rows, rows=rows)


_ORACLE = {}


def oracle(key, X, u_nom, bx, horizon=HOR):
    """One oracle run per set of inputs and test session."""
    if key not in _ORACLE:
        _ORACLE[key] = SC.solve_many(X, u_nom, np.broadcast_to(bx, (len(X),)).copy(), DT, horizon, SC.oracle_env(), SC.oracle_spec())
    return _ORACLE[key]


def hold(got, ref, cap, stored_eps=0.0, skip=()):
    """Every agent equals the oracle; returns how many were set aside (at most `cap`, each within the rule)."""
    flip, differs = SC.compare(got, ref, stored_eps)
    aside = flip & SC.may_set_aside(ref)
    bad = [i for i in np.flatnonzero(differs & ~aside) if i not in skip]
    print(f"set aside {int(aside.sum())} of {len(flip)} (cap {cap})")
    assert not bad, (bad[:8], [(got["status"][i], ref["status"][i], got["n_rows"][i], ref["n_rows"][i], got["u"][i], ref["u"][i]) for i in bad[:3]])
    assert aside.sum() <= cap
    return int(aside.sum())


def test_fixture_cases():
    """The reference's own single calls at scenario B."""
    got = solve(controller(float(GB["a_horizon"])), GB["a_X"], GB["a_u_nom"], GB["a_bullet_x"])
    n = GB["a_n_rows"]
    assert np.array_equal(got["n_rows"], n)
    assert np.array_equal(got["status"], GB["a_qp_status"])
    assert np.array_equal(got["using_backup"].astype(bool), GB["a_using_backup"])
    assert np.abs(got["h_min"] - GB["a_h_min"]).max() <= SC.H_TOL
    for i in range(len(n)):
        ref = GB["a_rows"][i][: n[i]]
        assert np.abs(got["rows"][i][: n[i]] - ref).max() <= SC.ROW_TOL * max(1.0, np.abs(ref).max()), i
    assert np.abs(got["u"] - GB["a_u"]).max() <= SC.U_TOL
    assert {(int(s), bool(b)) for s, b in zip(GB["a_qp_status"], GB["a_using_backup"])} == {(0, False), (0, True), (1, False), (1, True)}


@pytest.mark.parametrize("nominal", ["built_in", "user"])
def test_drawn_batch_against_oracle(nominal):
    B = SC.BATCH
    X, bx, u_user = SC.draw_states_b(B, SC.BATCH_SEED)
    u_nom = u_user if nominal == "user" else None
    ref = oracle(("batch", nominal), X, u_nom, bx)
    kinds = {(int(s), bool(b)) for s, b in zip(ref["status"], ref["using_backup"])}
    assert kinds == {(0, False), (0, True), (1, False), (1, True), (-1, False)}
    if nominal == "user":                                               # the no-rows branch returns the reference input unclipped
        none = ref["status"] == -1
        assert (np.abs(u_user[none]).max(axis=1) > SC.ROBOT["B"]["a_max"]).sum() >= 2 and np.array_equal(ref["u"][none], u_user[none])
    hold(solve(controller(), X, u_nom, bx), ref, cap=B // 100)


@pytest.mark.parametrize("bullet", ["per_agent", "shared"])
def test_f32_storage_against_oracle(bullet):
    """float32 storage, float64 arithmetic: the oracle on the rounded inputs, plus one float32 rounding of the stored u and h_min."""
    B = SC.BATCH
    X, bx, u_user = (a.astype(np.float32).astype(np.float64) for a in SC.draw_states_b(B, SC.BATCH_SEED))
    if bullet == "shared":
        bx = np.array([30.5])                                           # bullet_x[1]: one bullet for every agent
    ref = oracle(("f32", bullet), X, u_user, bx)
    got = solve(controller(io_dtype="f32"), X, u_user, bx)
    assert got["rows"].dtype == np.float64
    hold(got, ref, cap=B // 100, stored_eps=F32)
    assert len({(int(s), bool(b)) for s, b in zip(ref["status"], ref["using_backup"])}) >= 4


RAGGED = 65


@pytest.mark.parametrize("B", [1, 15, 17, RAGGED])
def test_ragged_batches(B):
    """Batch sizes that are no multiple of the 16 agents of a wave; the slot past the batch is not written."""
    X, bx, u_user = SC.draw_states_b(RAGGED, seed=5)
    ref = oracle("ragged", X, u_user, bx)
    ctl = controller()
    full = lambda shape, dt_: torch.full(shape, SENTINEL, dtype=dt_, device=DEV)
    out = (full((B + 1, 2), torch.float64), full((B + 1,), torch.int32), full((B + 1,), torch.int32), full((B + 1,), torch.float64),
           full((B + 1,), torch.int32), full((B + 1, ctl.N, 3), torch.float64))
    got = solve(ctl, X[:B], u_user[:B], bx[:B], out=out)
    hold(got, {k: v[:B] for k, v in ref.items()}, cap=B // 100)
    for a in out:
        assert bool((a[B] == SENTINEL).all())
    for i in range(B):                                                  # nor the rows past an agent's count
        assert bool((out[5][i, int(got["n_rows"][i]):] == SENTINEL).all())


@pytest.mark.parametrize("N,horizon", [(2, 0.2), (128, 12.8)])
def test_rollout_length_edges(N, horizon):
    """N = 2: one pass, the last-row branch fires at i = 1.  N = 128: the largest the entry point admits."""
    ctl = controller(horizon)
    p = BK.make_params(ctl.env, ctl.robot_spec, DT, horizon, _lib.DTYPE_F64)
    assert p.n_steps == N and ctl.N == N
    X, bx, u_user = SC.draw_states_b(32, seed=7 + N)
    ref = oracle(("edge", N), X, u_user, bx, horizon)
    assert ref["rows"].shape[1] == N and ref["n_rows"].max() > N // 2
    hold(solve(ctl, X, u_user, bx), ref, cap=0)


def test_poisoned_neighbour():
    """A NaN agent in the middle of a wave reports status 1 and leaves the other fifteen alone (the QP loop's exit is
    wave-uniform: a quad that is done at once must not cut the others short)."""
    X, bx, u_user = SC.draw_states_b(RAGGED, seed=5)
    ref = {k: v[:16] for k, v in oracle("ragged", X, u_user, bx).items()}
    X = X[:16].copy()
    X[7] = np.nan
    got = solve(controller(), X, u_user[:16], bx[:16])
    assert got["status"][7] == 1
    assert (ref["status"] == 0).sum() >= 3                                # some neighbours do walk the QP
    hold(got, ref, cap=0, skip=(7,))


LOOP_STEPS = 60


def loop_starts():
    X0, bx0 = SC.draw_loop_starts_b(32, seed=3)
    for i, tag in enumerate(("loopg", "looph", "loopr")):                 # the reference's recorded loops
        X0[i], bx0[i] = GB[f"{tag}_X"][0], GB[f"{tag}_bullet_x"][0]
    return X0, bx0


def test_closed_loops_against_oracle():
    """32 agents, 60 steps of the example's loop: outcome, its step, the bullet (respawn included) and the state, per agent."""
    B, T = 32, LOOP_STEPS
    X0, bx0 = loop_starts()
    if "loops" not in _ORACLE:
        _ORACLE["loops"] = SC.loops_many(X0, bx0, T, DT, HOR, SC.oracle_env(), SC.oracle_spec())
    o = _ORACLE["loops"]
    env = SC.oracle_env()
    n = o["n"]
    respawned = np.array([np.any(np.diff(o["bullet"][i][: n[i]]) < 0) for i in range(B)])
    assert (o["ret"] == 1).sum() >= 3 and (o["ret"] == -2).sum() >= 3 and (o["ret"] == 0).sum() >= 3 and respawned.sum() >= 2
    for i, tag in enumerate(("loopg", "looph", "loopr")):
        assert o["ret"][i] == int(GB[f"{tag}_outcome"])

    ctl = controller()
    X, bx = t(X0), t(bx0)
    ret = torch.zeros(B, dtype=torch.int32, device=DEV); rs = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    Xr, Br, Sr = [], [], []
    for k in range(T):                                                  # one step per launch: records the trajectories
        Xr.append(X.clone()); Br.append(bx.clone())
        Sr.append(ctl.rollout(X, bx, ret, rs, 1, step_offset=k)[1])
    Xf, bxf = t(X0), t(bx0)
    retf = torch.zeros(B, dtype=torch.int32, device=DEV); rsf = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    ctl.rollout(Xf, bxf, retf, rsf, T)
    torch.cuda.synchronize()
    assert torch.equal(Xf, X) and torch.equal(retf, ret) and torch.equal(rsf, rs) and torch.equal(bxf, bx)   # fused == per step, bit for bit
    Xr, Br, Sr = torch.stack(Xr).cpu().numpy(), torch.stack(Br).cpu().numpy(), torch.stack(Sr).cpu().numpy()
    Xe, be, ret, rs = X.cpu().numpy(), bx.cpu().numpy(), ret.cpu().numpy(), rs.cpu().numpy()

    aside = 0
    for i in range(B):
        m = n[i]
        b_end = o["bullet"][i][m - 1] + env["bullet_speed"] * DT          # EvadeEnv.step_bullet after the last recorded step
        if b_end > env["hallway_length"] + env["bullet_length"]:
            b_end = env["bullet_start_x"]
        ok = (ret[i], rs[i]) == (o["ret"][i], o["ret_step"][i])
        ok = ok and np.abs(Xr[:m, i] - o["X"][i][:m]).max() <= 1e-6 and np.abs(Br[:m, i] - o["bullet"][i][:m]).max() <= 1e-9
        ok = ok and np.abs(Xe[i] - o["x_final"][i]).max() <= 1e-6 and abs(be[i] - b_end) <= 1e-9
        if not ok:                                                      # excusable only as a status flip at a QP within 1e-6 of flipping
            k = int(np.argmax(Sr[:m, i] != o["status"][i][:m]))
            first = Sr[k, i] != o["status"][i][k] and np.abs(Xr[: k + 1, i] - o["X"][i][: k + 1]).max() <= 1e-6
            assert first and abs(o["margin"][i][k]) < 1e-6, (i, k, ret[i], rs[i], o["ret"][i], o["ret_step"][i])
            aside += 1
            continue
        if ret[i] != 0:                                                 # an agent that ended stays where it ended
            assert np.array_equal(Xr[rs[i] + 1:, i], np.broadcast_to(Xe[i], Xr[rs[i] + 1:, i].shape))
            assert np.array_equal(Br[rs[i] + 1:, i], np.broadcast_to(be[i], Br[rs[i] + 1:, i].shape))
    print(f"closed loops: set aside {aside} of {B}; goal {(o['ret'] == 1).sum()}, hit {(o['ret'] == -2).sum()}, running {(o['ret'] == 0).sum()}, "
          f"respawned {respawned.sum()}")
    assert aside <= 1
