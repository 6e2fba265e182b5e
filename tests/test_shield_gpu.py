"""GPU: Gatekeeper / MPS kernels (csrc/shield.hip) through the C-ABI against the reference-executed fixtures
(tests/golden/shield.npz) and the float64 oracle (tests/_shield_oracle.py).  The kernels repeat the reference's double
operations without contraction, so decisions are identical and states agree to rounding; a decision whose oracle margin is
within 1e-9 of a tie is counted, not compared.  The tests at the end repeat the fixture loop and the drawn batch at scenario B of
tests/_evade_scenarios.py (tests/golden/shield_b.npz), where no two scenario parameters are equal."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _shield_oracle as SO  # noqa: E402
import safe_control_amd as sca  # noqa: E402
from oracle import backup_cbf as OB  # noqa: E402

DEV = "cuda:0"
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "shield.npz"))
ALGOS = {"gatekeeper": SO.GATEKEEPER, "mps": SO.MPS}


def t(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def shield(algo, params=(0.1, 12.0, 10.0, 0.05), **kw):
    dt, bh, nh, eo = (float(v) for v in params)
    return sca.BatchedShield(algo, dt=dt, backup_horizon=bh, nominal_horizon=nh, event_offset=eo, **kw)


def draw(B, seed):
    """Situations of the kinds make_golden_shield.py draws (hallway with the bullet behind, below / in the pocket, bullet far
    or ahead, near the goal)."""
    rng = np.random.default_rng(seed)
    X = np.zeros((B, 4))
    bx = np.zeros(B)
    kind = np.arange(B) % 5
    u = lambda lo, hi: rng.uniform(lo, hi, B)
    x0, y0, vx0, vy0 = u(8, 50), u(-1.2, 1.2), u(0, 1.5), u(-0.3, 0.3)
    X[:] = np.column_stack([x0, y0, vx0, vy0])
    bx[:] = x0 - u(4, 14)
    m = kind == 1
    X[m] = np.column_stack([u(26.5, 33.5), u(-1.0, 1.4), u(-0.5, 1.0), u(-0.3, 0.8)])[m]
    bx[m] = X[m, 0] - u(3, 20)[m]
    m = kind == 2
    X[m] = np.column_stack([u(26.5, 33.5), u(2.8, 5.2), u(-0.4, 0.4), u(-0.4, 0.4)])[m]
    bx[m] = u(0, 60)[m]
    m = kind == 3
    X[m] = np.column_stack([u(5, 50), u(-1.0, 1.0), u(0.5, 1.5), u(-0.2, 0.2)])[m]
    bx[m] = np.where(u(0, 1) < 0.5, X[:, 0] + u(6, 20), -10.0)[m]
    m = kind == 4
    X[m] = np.column_stack([u(50, 58.5), u(-1.0, 1.0), u(0.0, 1.5), u(-0.2, 0.2)])[m]
    bx[m] = X[m, 0] - u(5, 30)[m]
    return X, bx


@pytest.mark.parametrize("algo", list(ALGOS))
@pytest.mark.parametrize("variant", ["base", "eo05", "bh2", "nh3", "dt005"])
def test_fixture_loop_as_agent_0(algo, variant):
    k = f"loop_{algo}_{variant}_"
    sh = shield(algo, G[k + "params"])
    B = 256
    X0, bx0 = draw(B, seed=5)
    X0[0], bx0[0] = (20.0, 0.0, 0.0, 0.0), -10.0                        # the example's start (test_evade.py:300-306)
    T = int(60.0 / float(G[k + "params"][0]))
    X, bx, st = t(X0), t(bx0), sh.new_state(B, DEV)
    ret = torch.zeros(B, dtype=torch.int32, device=DEV)
    rs = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    nb = torch.zeros(B, dtype=torch.int32, device=DEV)
    f = sh.fields(st, B)
    rec = []
    for step in range(T):
        x_pre = X[0].clone()
        u, using = sh.rollout(X, bx, st, ret, rs, 1, step_offset=step, backup_steps=nb)
        rec.append(torch.cat([x_pre, u[0], torch.stack([using[0], f["s"][0], f["idx"][0], f["clen"][0]]).double(), f["net"][:1]]))
    R = torch.stack(rec).cpu().numpy()
    n = len(G[k + "X"])
    assert (int(ret[0]), int(rs[0])) == (int(G[k + "outcome"]), int(G[k + "outcome_step"]))
    assert np.abs(R[:n, 0:4] - G[k + "X"]).max() <= 1e-9
    assert np.abs(R[:n, 4:6] - G[k + "U"]).max() <= 1e-9
    for j, g in ((6, "using_backup"), (7, "ans"), (8, "idx"), (9, "clen")):
        assert np.array_equal(R[:n, j].astype(np.int64), G[k + g].astype(np.int64)), g
    assert np.abs(R[:n, 10] - G[k + "net"]).max() <= 1e-12
    assert int(nb[0]) == int(G[k + "using_backup"].sum())
    # one fused launch from the same start: bit-identical to the per-step launches
    X2, bx2, st2 = t(X0), t(bx0), sh.new_state(B, DEV)
    ret2 = torch.zeros(B, dtype=torch.int32, device=DEV)
    rs2 = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    nb2 = torch.zeros(B, dtype=torch.int32, device=DEV)
    sh.rollout(X2, bx2, st2, ret2, rs2, T, backup_steps=nb2)
    for a, b in ((X, X2), (bx, bx2), (st, st2), (ret, ret2), (rs, rs2), (nb, nb2)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("algo", list(ALGOS))
def test_drawn_batch_against_oracle(algo):
    """4096 situations, four closed-loop warm-up steps each (commitments reached mid-run), then one call; 1024 of them
    replayed by the oracle."""
    B, W = 4096, 4
    X0, bx0 = draw(B, seed=11 + ALGOS[algo])
    sh = shield(algo)
    X, bx, st = t(X0), t(bx0), sh.new_state(B, DEV)
    ret = torch.zeros(B, dtype=torch.int32, device=DEV)
    rs = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    sh.rollout(X, bx, st, ret, rs, W)
    u, using, s = sh.step(X, bx, st)
    f = sh.fields(st, B)
    u, using, s, idx, clen, net, ret = (a.cpu().numpy() for a in (u, using, s, f["idx"], f["clen"], f["net"], ret))
    sub = np.arange(0, B, 4)
    o = SO.replay_many(ALGOS[algo], X0[sub], bx0[sub], W)
    ties = compared = 0
    kinds = set()
    for j, i in enumerate(sub):
        assert bool(ret[i]) == bool(o["ended"][j]), i
        if o["ended"][j]:
            continue
        if o["margin"][j] <= 1e-9:
            ties += 1
            continue
        compared += 1
        assert (s[i], idx[i], clen[i], bool(using[i])) == (o["s"][j], o["idx"][j], o["clen"][j], bool(o["using_backup"][j])), i
        assert abs(net[i] - o["net"][j]) <= 1e-12
        assert np.abs(u[i] - o["u"][j]).max() <= 1e-12, (i, u[i], o["u"][j])
        kinds.add((bool(o["s"][j] > 0), bool(o["found"][j]), bool(o["using_backup"][j])))
    assert compared >= 900
    assert ties <= 0.005 * len(sub)
    assert len(kinds) >= 3


def _nominal_rollout_batch(X, M, dt=0.1, vmax=1.5, amax=2.0):
    """The example's rollout_nominal for a batch, element for element the scalar operations of oracle.backup_cbf."""
    xs = np.zeros((len(X), M + 1, 4))
    us = np.zeros((len(X), M, 2))
    x = X.copy()
    xs[:, 0] = x
    for k in range(M):
        ax = 2.0 * (vmax - x[:, 2])
        ay = 2.0 * (0.0 - x[:, 1]) + 2.0 * (0.0 - x[:, 3])
        am = np.sqrt(ax ** 2 + ay ** 2)
        big = am > amax
        ax = np.where(big, ax * amax / np.where(big, am, 1.0), ax)
        ay = np.where(big, ay * amax / np.where(big, am, 1.0), ay)
        us[:, k, 0], us[:, k, 1] = ax, ay
        xn = np.column_stack([x[:, 0] + x[:, 2] * dt, x[:, 1] + x[:, 3] * dt, x[:, 2] + ax * dt, x[:, 3] + ay * dt])
        vm = np.sqrt(xn[:, 2] ** 2 + xn[:, 3] ** 2)
        big = vm > vmax
        sc = np.where(big, vmax / np.where(big, vm, 1.0), 1.0)
        xn[big, 2] *= sc[big]
        xn[big, 3] *= sc[big]
        x = xn
        xs[:, k + 1] = x
    return xs, us


@pytest.mark.parametrize("algo", list(ALGOS))
def test_device_nominal_equals_the_examples_rollout(algo):
    B = 512
    X0, bx0 = draw(B, seed=21)
    nx, nu = _nominal_rollout_batch(X0, 100)
    for i in (0, 7, 100):                                               # the batch form is the scalar rollout
        ox, ou = SO.nominal_rollout(X0[i], 100, OB.default_env(), OB.default_spec(), 0.1)
        assert np.array_equal(ox, nx[i]) and np.array_equal(ou, nu[i])
    sh = shield(algo)
    outs = []
    for nom in (None, (t(nx), t(nu))):
        st = sh.new_state(B, DEV)
        outs.append(sh.step(t(X0), t(bx0), st, *(nom or (None, None)), want_committed=True) + (st,))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))


@pytest.mark.parametrize("algo", list(ALGOS))
def test_f32_storage_makes_the_f64_decisions(algo):
    B = 1024
    X0, bx0 = draw(B, seed=31)
    X0, bx0 = X0.astype(np.float32).astype(np.float64), bx0.astype(np.float32).astype(np.float64)
    r = {}
    for io, dt_ in (("f64", torch.float64), ("f32", torch.float32)):
        sh = shield(algo, io_dtype=io)
        st = sh.new_state(B, DEV)
        u, using, s = sh.step(t(X0, dt_), t(bx0, dt_), st)
        r[io] = (u.double().cpu().numpy(), using.cpu().numpy(), s.cpu().numpy(), st.cpu().numpy())
    assert np.array_equal(r["f32"][1], r["f64"][1]) and np.array_equal(r["f32"][2], r["f64"][2])
    assert np.array_equal(r["f32"][3], r["f64"][3])                    # the state buffer is float64 either way
    assert np.abs(r["f32"][0] - r["f64"][0]).max() <= 1e-6


class _Env:
    """EvadeEnv's attributes and bullet (envs/evade_env.py:30-83,360-406) as the example builds it."""

    def __init__(self):
        e = OB.default_env()
        for k in ("hallway_length", "half_width", "pocket_x_min", "pocket_x_max", "pocket_y_min", "pocket_y_max", "goal_x_min", "goal_x_max",
                  "bullet_speed", "bullet_length", "bullet_width", "bullet_start_x"):
            setattr(self, k, e[k])
        self.bullet_x, self.bullet_active, self.bullet_vx = e["bullet_start_x"], True, e["bullet_speed"]

    def get_pocket_bounds(self):
        return {"x_min": self.pocket_x_min, "x_max": self.pocket_x_max, "y_min": self.pocket_y_min, "y_max": self.pocket_y_max}

    def get_bullet_state(self):
        return {"x": self.bullet_x + self.bullet_length / 6, "y": 0.0, "vx": self.bullet_vx, "vy": 0.0,
                "length": self.bullet_length * (1 + 1 / 3), "width": self.bullet_width, "active": self.bullet_active}

    def step_bullet(self, dt):
        self.bullet_x += self.bullet_vx * dt
        if self.bullet_x > self.hallway_length + self.bullet_length:
            self.bullet_x = self.bullet_start_x


class _Backup:
    def __init__(self, env):
        self.safe_center = np.array([(env.pocket_x_min + env.pocket_x_max) / 2, (env.pocket_y_min + env.pocket_y_max) / 2])
        self.safe_bounds = env.get_pocket_bounds()
        self.Kp, self.Kd, self.a_max, self.goal_bounds = 2.0, 2.0, 2.0, {}


def _compose(cls, variant="base", **kw):
    dt, bh, nh, eo = (float(v) for v in G[f"loop_gatekeeper_{variant}_params"])
    spec = {"radius": 0.5, "a_max": 2.0, "v_max": 1.5, "model": "DoubleIntegrator2D", "safety_margin": 0.5}
    env = _Env()
    args = dict(robot=None, robot_spec=spec, dt=dt, backup_horizon=bh, event_offset=eo, ax=None, safety_margin=0.5)
    if cls is sca.Gatekeeper:
        args["nominal_horizon"] = nh
    args.update(kw)
    sh = cls(**args)
    sh.set_backup_controller(_Backup(env))
    sh.set_environment(env)

    def get_obstacles(t=0.0):                                          # test_evade.py:373-384
        b = env.get_bullet_state()
        f = b.copy()
        f["x"] = b["x"] + b["vx"] * t
        return f

    sh.set_moving_obstacles(get_obstacles)
    return sh, env, dt, nh


@pytest.mark.parametrize("algo,variant", [("gatekeeper", "base"), ("gatekeeper", "bh2"), ("mps", "base")])
def test_dropins_reproduce_the_fixture_loops(algo, variant):
    """Driven exactly like test_evade.py:434-497."""
    k = f"loop_{algo}_{variant}_"
    sh, env, dt, nh = _compose(sca.Gatekeeper if algo == "gatekeeper" else sca.MPS, variant)
    spec, oenv = OB.default_spec(), OB.default_env()
    state = np.array([20.0, 0.0, 0.0, 0.0]).reshape(-1, 1)
    outcome, out_step, backup = 0, -1, 0
    for step in range(int(60.0 / dt)):
        pos = state[:2, 0].copy()
        nx, nu = SO.nominal_rollout(state.flatten(), int(nh / dt), oenv, spec, dt)
        sh.set_nominal_trajectory(nx, nu)
        control = sh.solve_control_problem(state)
        assert np.abs(control.flatten() - G[k + "U"][step]).max() <= 1e-12, step
        st = sh.get_status()
        assert (sh.is_using_backup(), sh.actual_nominal_steps, st["current_time_idx"], st["committed_length"]) == (
            G[k + "using_backup"][step], G[k + "ans"][step], G[k + "idx"][step], G[k + "clen"][step]), step
        backup += sh.is_using_backup()
        state = OB.di_step(state.flatten(), control.flatten(), dt, 1.5).reshape(-1, 1)
        vm = np.sqrt(state[2, 0] ** 2 + state[3, 0] ** 2)
        if vm > 1.5:
            state[2, 0], state[3, 0] = state[2, 0] * 1.5 / vm, state[3, 0] * 1.5 / vm
        env.step_bullet(dt)
        if OB.bullet_hits(pos, env.bullet_x, oenv, 0.5):
            outcome, out_step = -2, step
            break
        if oenv["goal_x_min"] <= pos[0] <= oenv["goal_x_max"] and -2.0 <= pos[1] <= 2.0:
            outcome, out_step = 1, step
            break
    assert (outcome, out_step) == (int(G[k + "outcome"]), int(G[k + "outcome_step"]))
    cx, cu = sh.get_committed_trajectory()
    assert cx.shape == (len(cu) + 1, 4) and len(cu) == sh.get_status()["committed_length"]
    assert sh.get_committed_horizon() == sh.actual_nominal_steps * dt


def test_dropin_committed_trajectory_matches_the_single_calls():
    k = "calls_gatekeeper_"
    spec, oenv = OB.default_spec(), OB.default_env()
    for i in range(0, len(G[k + "X"]), 3):
        sh, env, dt, nh = _compose(sca.Gatekeeper)
        env.bullet_x = float(G[k + "bullet_x"][i])
        sh.set_nominal_trajectory(*SO.nominal_rollout(G[k + "X"][i], 100, oenv, spec, dt))
        sh.solve_control_problem(G[k + "X"][i])
        cx, cu = sh.get_committed_trajectory()
        n = int(G[k + "clen"][i])
        assert np.abs(cx - G[k + "cx"][i][:n + 1]).max() <= 1e-12 and np.abs(cu - G[k + "cu"][i][:n]).max() <= 1e-12, i


def test_refused_compositions_raise():
    with pytest.raises(NotImplementedError):
        sca.Gatekeeper(None, {"model": "DynamicBicycle2D"})
    sh, env, dt, nh = _compose(sca.Gatekeeper)
    with pytest.raises(NotImplementedError):
        sh.set_backup_controller(object())
    sh.set_nominal_controller(lambda x: np.zeros((2, 1)))                   # forward-propagation mode
    with pytest.raises(NotImplementedError):
        sh.solve_control_problem(np.array([20.0, 0.0, 0.0, 0.0]))
    sh, env, dt, nh = _compose(sca.MPS)
    sh.set_nominal_trajectory(*SO.nominal_rollout(np.array([20.0, 0, 0, 0]), 100, OB.default_env(), OB.default_spec(), dt))
    sh.set_moving_obstacles(lambda t=0.0: {"x": 0.0, "y": 0.0, "length": 1.0, "width": 1.0, "vx": 0.0})
    with pytest.raises(NotImplementedError):
        sh.solve_control_problem(np.array([20.0, 0.0, 0.0, 0.0]))
    with pytest.raises(NotImplementedError):
        sca.BatchedShield("gatekeeper", robot_spec={"model": "Quad3D"})


def test_argument_validation():
    sh = shield("gatekeeper")
    st = sh.new_state(4, DEV)
    X, bx = t(np.zeros((4, 4))), t(np.zeros(4))
    with pytest.raises(ValueError):
        sh.step(X.float(), bx, st)                                        # dtype
    with pytest.raises(ValueError):
        sh.step(X, bx, sh.new_state(3, DEV))                              # state of another batch size
    with pytest.raises(ValueError):
        sh.step(X, bx, st, t(np.zeros((4, 11, 4))), t(np.zeros((4, 9, 2))))
    with pytest.raises(ValueError):
        sca.BatchedShield("cbf")
    ret = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        sh.rollout(X, bx[:1], st, ret, ret.clone(), 1)


# ---- scenario B (tests/_evade_scenarios.py): no two parameters equal, so a wrong field in shield.hip, evade.hpp or the parameter
# fill of BatchedShield shows ------------------------------------------------------------------------------------------------
import _evade_scenarios as SC  # noqa: E402

GB = np.load(os.path.join(os.path.dirname(__file__), "golden", "shield_b.npz"))


def shield_b(algo):
    dt, bh, nh, eo = (float(v) for v in GB[f"loop_{algo}_base_params"])
    rb = SC.ROBOT["B"]
    return sca.BatchedShield(algo, robot_spec={k: rb[k] for k in ("radius", "a_max", "v_max")}, env=SC.kernel_env("B"), dt=dt,
                             backup_horizon=bh, nominal_horizon=nh, event_offset=eo, safety_margin=rb["safety_margin"],
                             kp=SC.GAINS["B"]["kp"], kd=SC.GAINS["B"]["kd"])


@pytest.mark.parametrize("algo", list(ALGOS))
def test_scenario_b_fixture_loop_as_agent_0(algo):
    k = f"loop_{algo}_base_"
    sh = shield_b(algo)
    B = 256
    X0, bx0 = SC.draw_calls_b(B, seed=5)
    X0[0], bx0[0] = GB[k + "X"][0], GB[k + "bullet_x"][0]
    T = n = len(GB[k + "X"])
    X, bx, st = t(X0), t(bx0), sh.new_state(B, DEV)
    ret = torch.zeros(B, dtype=torch.int32, device=DEV)
    rs = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    nb = torch.zeros(B, dtype=torch.int32, device=DEV)
    f = sh.fields(st, B)
    rec = []
    for step in range(T):
        x_pre, b_pre = X[0].clone(), bx[:1].clone()
        u, using = sh.rollout(X, bx, st, ret, rs, 1, step_offset=step, backup_steps=nb)
        rec.append(torch.cat([x_pre, u[0], torch.stack([using[0], f["s"][0], f["idx"][0], f["clen"][0]]).double(), f["net"][:1], b_pre]))
    R = torch.stack(rec).cpu().numpy()
    assert (int(ret[0]), int(rs[0])) == (int(GB[k + "outcome"]), int(GB[k + "outcome_step"]))
    assert np.abs(R[:n, 0:4] - GB[k + "X"]).max() <= 1e-9
    assert np.abs(R[:n, 4:6] - GB[k + "U"]).max() <= 1e-9
    for j, g in ((6, "using_backup"), (7, "ans"), (8, "idx"), (9, "clen")):
        assert np.array_equal(R[:n, j].astype(np.int64), GB[k + g].astype(np.int64)), g
    assert np.abs(R[:n, 10] - GB[k + "net"]).max() <= 1e-12
    assert np.abs(R[:n, 11] - GB[k + "bullet_x"]).max() <= 1e-9
    assert int(nb[0]) == int(GB[k + "using_backup"].sum())
    X2, bx2, st2 = t(X0), t(bx0), sh.new_state(B, DEV)
    ret2 = torch.zeros(B, dtype=torch.int32, device=DEV)
    rs2 = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    nb2 = torch.zeros(B, dtype=torch.int32, device=DEV)
    sh.rollout(X2, bx2, st2, ret2, rs2, T, backup_steps=nb2)
    for a, b in ((X, X2), (bx, bx2), (st, st2), (ret, ret2), (rs, rs2), (nb, nb2)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("algo", list(ALGOS))
def test_scenario_b_drawn_batch_against_oracle(algo):
    """test_drawn_batch_against_oracle at scenario B: 1024 situations, four warm-up steps, one call; 256 replayed by the oracle."""
    B, W = 1024, 4
    X0, bx0 = SC.draw_calls_b(B, seed=11 + ALGOS[algo])
    sh = shield_b(algo)
    X, bx, st = t(X0), t(bx0), sh.new_state(B, DEV)
    ret = torch.zeros(B, dtype=torch.int32, device=DEV)
    rs = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    sh.rollout(X, bx, st, ret, rs, W)
    u, using, s = sh.step(X, bx, st)
    f = sh.fields(st, B)
    u, using, s, idx, clen, net, ret = (a.cpu().numpy() for a in (u, using, s, f["idx"], f["clen"], f["net"], ret))
    sub = np.arange(0, B, 4)
    o = SO.replay_many(ALGOS[algo], X0[sub], bx0[sub], W, params=tuple(float(v) for v in GB[f"loop_{algo}_base_params"]),
                       env=SC.oracle_env(), spec=SC.oracle_spec())
    ties = compared = 0
    kinds = set()
    for j, i in enumerate(sub):
        assert bool(ret[i]) == bool(o["ended"][j]), i
        if o["ended"][j]:
            continue
        if o["margin"][j] <= 1e-9:
            ties += 1
            continue
        compared += 1
        assert (s[i], idx[i], clen[i], bool(using[i])) == (o["s"][j], o["idx"][j], o["clen"][j], bool(o["using_backup"][j])), i
        assert abs(net[i] - o["net"][j]) <= 1e-12
        assert np.abs(u[i] - o["u"][j]).max() <= 1e-12, (i, u[i], o["u"][j])
        kinds.add((bool(o["s"][j] > 0), bool(o["found"][j]), bool(o["using_backup"][j])))
    print(f"{algo}: compared {compared}, ties {ties} of {len(sub)}")
    # The warm-up ends the agents drawn inside the goal zone (half of the one kind in five drawn around its edge, 10 %) and those
    # the bullet reaches within four steps (nose gaps below ~1.7 m among the two kinds drawn with the bullet close behind, ~5 %).
    assert compared >= 0.8 * len(sub)
    assert ties <= 0.005 * len(sub)
    assert len(kinds) >= 3
