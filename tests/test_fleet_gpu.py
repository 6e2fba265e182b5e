"""GPU tests: the fleet closed loop (BatchedFleetTrackingController, sc_tracking_fleet_step_batch), agents that are each
other's moving obstacles, against the fleet oracle (tests/_fleet_oracle.py).

Also the per-rank worker of the sharded test: ``python -m torch.distributed.run --nproc-per-node 2 tests/test_fleet_gpu.py
OUT.npz N_AGENTS STEPS`` (gloo, both ranks on the one GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import _fleet_oracle as FO  # noqa: E402
import safe_control_amd as sca  # noqa: E402
from safe_control_amd import workloads as W  # noqa: E402

DEV = "cuda:0"
C3BF = {"model": "KinematicBicycle2D_C3BF"}


def _np(t):
    return t.double().cpu().numpy() if t.is_floating_point() else t.cpu().numpy()


# ---- closed-loop oracle runs: started once, in plain child processes, while the GPU tests run -------------------------
_LOOPS = {
    "c3bf": dict(model="KinematicBicycle2D_C3BF", n=96, m=8, steps=200, seed=3),
    "dpcbf": dict(model="KinematicBicycle2D_DPCBF", n=64, m=8, steps=150, seed=5),
    "du": dict(model="DynamicUnicycle2D", n=64, m=8, steps=150, seed=7, goal_dist=(2.0, 6.0), spacing=2.0),
}


def _scene(cfg):
    X0, wps, obs = W.kb_c3bf_fleet_scene(cfg["n"], cfg["m"], seed=cfg["seed"], spec={"model": cfg["model"]},
                                         spacing=cfg.get("spacing", 3.0), goal_dist=cfg.get("goal_dist", (10.0, 20.0)))
    if cfg["model"] == "DynamicUnicycle2D":
        X0[:, 3] = np.minimum(X0[:, 3], 1.0)                  # v_max = 1
    return X0, wps, obs


@pytest.fixture(scope="module")
def loop_oracles():
    keys = list(_LOOPS)
    jobs = []
    for k in keys:
        cfg = _LOOPS[k]
        X0, wps, obs = _scene(cfg)
        jobs.append(dict(model=cfg["model"], spec={"model": cfg["model"]}, X0=X0, waypoints=wps, obs=obs, dyn_obs=True,
                         K_nb=16, num_constraints=10, steps=cfg["steps"]))
    h = FO.start_many(jobs)
    res = {}

    def get(k):
        if not res:
            res.update(zip(keys, FO.collect_many(h)))
        return res[k]
    yield get
    if not res:
        FO.collect_many(h)


# ---- one step, mixed states ------------------------------------------------------------------------------------------
def _mixed_fleet(io):
    """4096 C3BF agents scattered so that neighbours come at every distance (some overlap), an 8-row moving table,
    states track / stop / rotate, some agents frozen (-1 / -2), some standing still (degenerate C3BF rows)."""
    rng = np.random.default_rng(11)
    n = 4096
    X0 = np.column_stack([rng.uniform(0, 64, n), rng.uniform(0, 64, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(0.2, 3.0, n)])
    X0[rng.random(n) < 0.03, 3] = 0.0
    wps = [rng.uniform(0, 64, (int(rng.integers(1, 4)), 2)) for _ in range(n)]
    obs = np.zeros((8, 7))
    obs[:, 0:2] = rng.uniform(0, 64, (8, 2)); obs[:, 2] = 0.5; obs[:, 3:5] = rng.uniform(-0.5, 0.5, (8, 2))
    if io == "f32":
        X0, obs = X0.astype(np.float32).astype(np.float64), obs.astype(np.float32).astype(np.float64)
        wps = [w.astype(np.float32).astype(np.float64) for w in wps]
    rot = rng.random(n) < 0.15
    frozen = np.where(rng.random(n) < 0.05, np.where(rng.random(n) < 0.5, -1, -2), 0)
    return X0, wps, obs, rot, frozen


@pytest.mark.parametrize("io,tol", [("f64", 1e-9), ("f32", 1e-5)])
def test_one_step_mixed_states_against_oracle(io, tol):
    X0, wps, obs, rot, frozen = _mixed_fleet(io)
    n = len(X0)
    ctl = sca.BatchedFleetTrackingController(X0, dict(C3BF), obs=obs, dyn_obs=True, neighbours=16, io_dtype=io, device=DEV)
    ctl.set_waypoints(wps)
    orc = FO.FleetOracle("KinematicBicycle2D_C3BF", X0, dict(C3BF), wps, obs=obs, dyn_obs=True, K_nb=16,
                         io=np.float32 if io == "f32" else np.float64)
    sm = _np(ctl.state_machine)
    sm_o = np.array([{"idle": 0, "track": 1, "stop": 2, "rotate": 3}[a.state_machine] for a in orc.agents])
    np.testing.assert_array_equal(sm, sm_o)                   # set_waypoints: track / stop by field of view
    goal = _np(ctl.goal)
    for i in np.nonzero(rot & (sm != 0))[0]:                  # some agents with a goal turn on the spot towards their waypoint
        a = orc.agents[i]
        w = a.waypoints[a.current_goal_index] if a.current_goal_index < len(a.waypoints) else a.waypoints[-1]
        a.state_machine, a.goal = "rotate", np.array(w[:2])
        sm[i] = 3; goal[i] = [w[0], w[1], 1.0]
    ctl.state_machine.copy_(torch.tensor(sm, dtype=torch.int32))
    ctl.goal.copy_(torch.tensor(goal))
    orc.ret[:] = frozen; orc.ret_step[frozen != 0] = 0
    ctl.ret.copy_(torch.tensor(frozen, dtype=torch.int32))
    ctl.ret_step.copy_(torch.tensor(np.where(frozen != 0, 0, -1), dtype=torch.int32))
    ctl.X_pub[torch.tensor(frozen != 0, device=DEV), 3] = 0.0
    ctl.steps_done = 1
    orc.t = 1
    assert (sm == 1).any() and (sm == 2).any() and (sm == 3).any()

    ctl.control_step(1)
    orc.step()
    o = orc.state()
    ret, cause = _np(ctl.ret), _np(ctl.cause)
    assert {-2, -1, 0} <= set(o["ret"].tolist()) and {1, 2} <= set(o["cause"].tolist())
    if io == "f64":
        np.testing.assert_array_equal(ret, o["ret"])
        np.testing.assert_array_equal(cause, o["cause"])
        np.testing.assert_array_equal(_np(ctl.state_machine), o["sm"])
        np.testing.assert_array_equal(_np(ctl.current_goal_index), o["wp"])
        same = np.ones(n, dtype=bool)
    else:                                                     # storage rounding may tip a decision at a threshold
        same = (ret == o["ret"]) & (cause == o["cause"])
        assert same.mean() >= 0.999
        assert (_np(ctl.state_machine) == o["sm"]).mean() >= 0.999
    if io == "f64":
        np.testing.assert_array_equal(_np(ctl.ret_step), o["ret_step"])
    np.testing.assert_allclose(_np(ctl.X)[same], o["X"][same], rtol=tol, atol=tol)
    never = np.isnan(o["u"][:, 0])                            # the oracle's u_pos is None until the robot first moves
    np.testing.assert_allclose(_np(ctl.u_pos)[same & ~never], o["u"][same & ~never], rtol=tol, atol=tol)
    assert np.all(_np(ctl.u_pos)[same & never] == 0.0)
    ms, mso = _np(ctl.min_sep), o["min_sep"]
    np.testing.assert_array_equal(np.isinf(ms), np.isinf(mso))
    fin = np.isfinite(mso)
    np.testing.assert_allclose(ms[fin], mso[fin], rtol=0, atol=tol)
    # the published states: positions of every agent, speed 0 for the frozen ones
    pub = _np(ctl.X_pub)
    np.testing.assert_array_equal(pub[:, :3], _np(ctl.X)[:, :3])
    assert np.all(pub[ret != 0, 3] == 0) and np.all(pub[ret == 0, 3] == _np(ctl.X)[ret == 0, 3])


# ---- every kernel the fleet step's dispatch can select --------------------------------------------------------------------
@pytest.mark.parametrize("io,tol", [("f64", 1e-9), ("f32", 1e-5)])           # the one-step figures of the test above
@pytest.mark.parametrize("num_constraints", [8, 9], ids=["8_lanes_per_agent", "16_lanes_per_agent"])
@pytest.mark.parametrize("model", sca.BatchedFleetTrackingController.MODELS)
def test_every_kernel_of_the_fleet_dispatch(model, num_constraints, io, tol):
    """tracking_fleet_kernel with 8 lanes per agent (num_constraints <= 8 and M + K_nb <= 32) and with 16, for every model and
    storage type: 65 agents (a partial last block in both forms), a 3-row moving table, 8 neighbours, one step against the oracle."""
    cfg = dict(model=model, n=65, m=3, seed=21, **({"goal_dist": (2.0, 6.0), "spacing": 2.0} if model == "DynamicUnicycle2D" else {}))
    X0, wps, obs = _scene(cfg)
    wps = list(wps)
    if io == "f32":
        X0, obs = X0.astype(np.float32).astype(np.float64), obs.astype(np.float32).astype(np.float64)
        wps = [np.asarray(w).astype(np.float32).astype(np.float64) for w in wps]
    spec = {"model": model}
    ctl = sca.BatchedFleetTrackingController(X0, dict(spec), obs=obs, dyn_obs=True, neighbours=8, num_constraints=num_constraints,
                                             io_dtype=io, device=DEV)
    ctl.set_waypoints(wps)
    orc = FO.FleetOracle(model, X0, dict(spec), wps, obs=obs, dyn_obs=True, K_nb=8, num_constraints=num_constraints,
                         io=np.float32 if io == "f32" else np.float64)
    ctl.control_step(1)
    orc.step()
    o = orc.state()
    np.testing.assert_array_equal(_np(ctl.ret), o["ret"])
    np.testing.assert_array_equal(_np(ctl.cause), o["cause"])
    np.testing.assert_array_equal(_np(ctl.state_machine), o["sm"])
    np.testing.assert_allclose(_np(ctl.X), o["X"], rtol=tol, atol=tol)
    fin = np.isfinite(o["min_sep"])
    np.testing.assert_array_equal(np.isinf(_np(ctl.min_sep)), ~fin)
    np.testing.assert_allclose(_np(ctl.min_sep)[fin], o["min_sep"][fin], rtol=0, atol=tol)


# ---- closed loops -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(_LOOPS))
def test_closed_loop_against_oracle(key, loop_oracles):
    cfg = _LOOPS[key]
    X0, wps, obs = _scene(cfg)
    ctl = sca.BatchedFleetTrackingController(X0, {"model": cfg["model"]}, obs=obs, dyn_obs=True, neighbours=16, io_dtype="f64", device=DEV)
    ctl.set_waypoints(list(wps))
    _, tX, _ = ctl.control_step(cfg["steps"], record=True)
    o = loop_oracles(key)
    np.testing.assert_allclose(_np(tX), o["traj"], rtol=1e-6, atol=1e-6)   # every state after every step
    np.testing.assert_allclose(_np(ctl.X), o["X"], rtol=1e-6, atol=1e-6)
    np.testing.assert_array_equal(_np(ctl.ret), o["ret"])
    np.testing.assert_array_equal(_np(ctl.ret_step), o["ret_step"])
    np.testing.assert_array_equal(_np(ctl.cause), o["cause"])
    fin = np.isfinite(o["min_sep"])
    np.testing.assert_allclose(_np(ctl.min_sep)[fin], o["min_sep"][fin], rtol=0, atol=1e-6)
    s = ctl.summary()
    assert s["running"] + s["reached"] + s["infeasible"] + s["collided"] == cfg["n"]
    assert s["reached"] == int((o["ret"] == -1).sum()) and s["infeasible"] == int((o["cause"] == 1).sum())
    if key == "c3bf":
        assert (o["ret"] == -1).any() and (o["ret"] == -2).any()


# ---- sharding: two ranks equal one process bit for bit ------------------------------------------------------------------
def _shard_run(n_agents, steps):
    X0, wps, obs = W.kb_c3bf_fleet_scene(n_agents, 16, seed=9)
    ctl = sca.BatchedFleetTrackingController(X0, dict(C3BF), obs=obs, dyn_obs=True, neighbours=16, io_dtype="f64", device=DEV)
    ctl.set_waypoints(list(wps))
    ctl.control_step(steps)
    torch.cuda.synchronize()
    return ctl


@pytest.mark.parametrize("n_agents", [2048, 2047])
def test_two_ranks_equal_one_process_bitwise(tmp_path, n_agents):
    steps = 50
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / "rank.npz"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(29541 + n_agents % 2), os.path.abspath(__file__),
                        str(out), str(n_agents), str(steps)], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    parts = [np.load(str(out) + f".{k}.npz") for k in range(2)]
    ctl = _shard_run(n_agents, steps)
    for name, t in (("X", ctl.X), ("ret", ctl.ret), ("ret_step", ctl.ret_step), ("cause", ctl.cause), ("min_sep", ctl.min_sep)):
        got = np.concatenate([p[name] for p in parts])
        np.testing.assert_array_equal(got, t.cpu().numpy(), err_msg=name)
    s1 = ctl.summary()
    assert all(int(p["summary"][0]) == s1["running"] and int(p["summary"][3]) == s1["collided"] for p in parts)


def _rank_main(out, n_agents, steps):
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    ctl = _shard_run(n_agents, steps)
    s = ctl.summary()
    np.savez(out + f".{dist.get_rank()}.npz", X=ctl.X.cpu().numpy(), ret=ctl.ret.cpu().numpy(), ret_step=ctl.ret_step.cpu().numpy(),
             cause=ctl.cause.cpu().numpy(), min_sep=ctl.min_sep.cpu().numpy(),
             summary=np.array([s["running"], s["reached"], s["infeasible"], s["collided"]]))
    dist.barrier()
    dist.destroy_process_group()


# ---- BASELINE configs[3] size ---------------------------------------------------------------------------------------------
def test_configs3_size_16384_agents_f32():
    n, steps = 16384, 200
    X0, wps, obs = W.kb_c3bf_fleet_scene(n, 16, seed=0)
    runs = []
    for _ in range(2):
        ctl = sca.BatchedFleetTrackingController(X0, dict(C3BF), obs=obs, dyn_obs=True, neighbours=16, io_dtype="f32", device=DEV)
        ctl.set_waypoints(list(wps))
        ctl.control_step(steps)
        runs.append((ctl.X.cpu().numpy(), ctl.ret.cpu().numpy(), ctl.cause.cpu().numpy(), ctl.min_sep.cpu().numpy(), ctl.summary()))
    (X, ret, cause, ms, s), (X2, ret2, cause2, ms2, _) = runs
    np.testing.assert_array_equal(X, X2)
    np.testing.assert_array_equal(ret, ret2)
    np.testing.assert_array_equal(cause, cause2)
    np.testing.assert_array_equal(ms, ms2)
    assert np.isfinite(X[ret == 0]).all()
    assert s["running"] + s["reached"] + s["infeasible"] + s["collided"] == n
    assert s["reached"] > 0
    assert np.all(ret[ms < 0] == -2)
    assert s["min_sep"] == pytest.approx(float(ms.min()))


if __name__ == "__main__":
    _rank_main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
