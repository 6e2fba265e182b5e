"""Cases of the per-agent parameter tests (tests/test_agent_params_abi.py, tests/test_agent_params_gpu.py): seeded draws of
heterogeneous batches, and their oracles -- the existing single-agent oracles called once per agent with that agent's spec.

The seeds below were chosen on the CPU by ``python tests/_agent_params_cases.py`` (oracle only, no GPU):
  * solve cases: the first seed whose batch holds both 'optimal' and 'infeasible' agents and no agent whose feasibility margin
    (oracle/qp.py: feasibility_margin, the Chebyshev LP the existing CBF-QP tests use) is within 1e-4 of zero, so that status
    equality of every agent is decided away from rounding;
  * closed-loop cases: the first seed for which -1, -2 and 0 all occur among the oracle's return codes AND the return codes and
    finishing steps of every agent are unchanged when every start state is moved by +1e-12 and by -1e-12 (no decision of the
    run -- waypoint reached, obstacle in the unpassed cone, collision, active set -- sits on a tie).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import cbf_qp as ocbf, qp as oqp, robots as R, tracking  # noqa: E402

SOLVE_MODELS = ("DynamicUnicycle2D", "KinematicBicycle2D", "KinematicBicycle2D_C3BF", "KinematicBicycle2D_DPCBF", "Unicycle2D",
                "SingleIntegrator2D", "DoubleIntegrator2D")
KB_FAMILY = ("KinematicBicycle2D", "KinematicBicycle2D_C3BF", "KinematicBicycle2D_DPCBF")
DT = 0.05


def model_id(name):
    return R.MODEL_NAMES[name]


def draw_agent_specs(name, B, rng):
    """One robot_spec per agent with EVERY key that may vary drawn per agent (those the model reads)."""
    specs = []
    for _ in range(B):
        s = {"model": name, "radius": float(rng.uniform(0.2, 0.35)), "reached_threshold": float(rng.uniform(0.2, 0.5)),
             "fov_angle": float(rng.uniform(50.0, 120.0))}
        if name == "DynamicUnicycle2D":
            s.update(a_max=float(rng.uniform(0.5, 1.5)), w_max=float(rng.uniform(0.4, 1.0)), v_max=float(rng.uniform(0.8, 2.0)))
        elif name in KB_FAMILY:
            s.update(a_max=float(rng.uniform(2.0, 5.0)), v_max=float(rng.uniform(2.5, 3.5)), v_min=float(rng.uniform(0.1, 0.3)),
                     beta_max=float(rng.uniform(0.2, 0.3)))
        elif name == "Unicycle2D":
            s.update(v_max=float(rng.uniform(0.8, 2.0)), w_max=float(rng.uniform(0.4, 1.0)))
        elif name == "SingleIntegrator2D":
            s.update(v_max=float(rng.uniform(0.8, 2.0)))
        else:
            s.update(a_max=float(rng.uniform(0.5, 1.5)), v_max=float(rng.uniform(0.8, 2.0)))
        if model_id(name) in R.REL_DEG2:
            s.update(cbf_alpha1=float(rng.uniform(0.5, 3.0)), cbf_alpha2=float(rng.uniform(0.5, 3.0)))
        else:
            s.update(cbf_alpha=float(rng.uniform(0.5, 3.0)))
        specs.append(s)
    return specs


def oracle_args(spec):
    """``(model id, oracle spec, cbf_param)`` of one agent's robot_spec: what the single-agent oracles take."""
    m = model_id(spec["model"])
    ospec = R.default_spec(m)
    ospec.update({k: v for k, v in spec.items() if k not in ("model", "cbf_alpha", "cbf_alpha1", "cbf_alpha2", "num_constraints")})
    cp = ocbf.default_cbf_param(m)
    for key, src in (("alpha", "cbf_alpha"), ("alpha1", "cbf_alpha1"), ("alpha2", "cbf_alpha2")):
        if src in spec and key in cp:
            cp[key] = float(spec[src])
    return m, ospec, cp


# ---- solve ---------------------------------------------------------------------------------------------------------------
def solve_case(name, K, shared, seed, B=67):
    """B agents of ``name`` with their own specs, states, references, ``n_obs`` in [0, K] and obstacles ``[B,K,7]`` (placed around
    each agent) or one shared ``[K,7]`` table."""
    rng = np.random.default_rng(seed)
    specs = draw_agent_specs(name, B, rng)
    m = model_id(name)
    X = np.zeros((B, 4))
    X[:, 0:2] = rng.uniform(0.0, 14.0, (B, 2))
    if m == R.MODEL_DI:
        X[:, 2:4] = rng.uniform(-1.0, 1.0, (B, 2))
    elif m != R.MODEL_SI:
        X[:, 2] = rng.uniform(-np.pi, np.pi, B)
        if m != R.MODEL_UNI:
            X[:, 3] = rng.uniform(0.2, 3.0, B) if name in KB_FAMILY else rng.uniform(0.0, 1.5, B)
    moving = name in ("KinematicBicycle2D_C3BF", "KinematicBicycle2D_DPCBF")
    if shared:
        obs = np.zeros((K, 7))
        obs[:, 0:2] = rng.uniform(0.0, 14.0, (K, 2))
        obs[:, 2] = rng.uniform(0.2, 0.6, K)
        if moving:
            obs[:, 3:5] = rng.uniform(-0.5, 0.5, (K, 2))
        # an agent inside an obstacle of the shared table is moved out of it: the barriers' square roots need h defined
        for i in range(B):
            for _ in range(50):
                d = np.hypot(obs[:, 0] - X[i, 0], obs[:, 1] - X[i, 1]) - obs[:, 2] - 0.35 - 0.4
                if d.min() > 0:
                    break
                X[i, 0:2] = rng.uniform(0.0, 14.0, 2)
    else:
        r = rng.uniform(0.2, 0.8, (B, K))
        rho = r + 0.35 + 0.4 + rng.uniform(0.0, 1.0, (B, K)) ** 2 * 4.0
        phi = rng.uniform(-np.pi, np.pi, (B, K))
        obs = np.zeros((B, K, 7))
        obs[:, :, 0] = X[:, None, 0] + rho * np.cos(phi)
        obs[:, :, 1] = X[:, None, 1] + rho * np.sin(phi)
        obs[:, :, 2] = r
        if moving:
            obs[:, :, 3:5] = rng.uniform(-0.5, 0.5, (B, K, 2))
    n_obs = rng.integers(0, K + 1, B).astype(np.int32)
    # the first four agents stand well inside one of their obstacles: the relative-degree-1 barriers (Unicycle2D, SingleIntegrator2D)
    # turn infeasible only there, and every case is to hold both statuses
    for i in range(4):
        frac, ang = rng.uniform(0.2, 0.6), rng.uniform(-np.pi, np.pi)
        if shared:
            j = i % K
            X[i, 0:2] = obs[j, 0:2] + frac * (obs[j, 2] + 0.2) * np.array([np.cos(ang), np.sin(ang)])
            n_obs[i] = K
        else:
            obs[i, 0, 0:2] = X[i, 0:2] + frac * (obs[i, 0, 2] + 0.2) * np.array([np.cos(ang), np.sin(ang)])
            n_obs[i] = max(int(n_obs[i]), 1)
    goal = rng.uniform(0.0, 14.0, (B, 2))
    u_ref = np.zeros((B, 2))
    for i in range(B):
        mi, ospec, _ = oracle_args(specs[i])
        u_ref[i] = R.nominal_input(mi, X[i], goal[i], ospec)
    return dict(name=name, K=K, shared=shared, specs=specs, X=X, u_ref=u_ref, obs=obs, n_obs=n_obs)


def oracle_solve(case, X=None, u_ref=None, obs=None, margins=False):
    """The existing oracle, once per agent with that agent's spec.  ``X`` / ``u_ref`` / ``obs``: the storage-rounded arrays the
    kernel saw, where they differ from the case's.  Returns ``u [B,2]`` (NaN where not optimal), ``status [B]``, ``h [B,K]`` (0 in
    unused rows, as the kernels write it) and, with ``margins`` (the seed search), the feasibility margin of every agent."""
    X = case["X"] if X is None else X
    u_ref = case["u_ref"] if u_ref is None else u_ref
    obs = case["obs"] if obs is None else obs
    B, K = X.shape[0], case["K"]
    u = np.full((B, 2), np.nan); st = np.zeros(B, dtype=np.int32); h = np.zeros((B, K)); mg = np.zeros(B)
    for i in range(B):
        m, ospec, cp = oracle_args(case["specs"][i])
        o = obs if obs.ndim == 2 else obs[i]
        k = int(case["n_obs"][i])
        r = ocbf.solve(m, X[i], u_ref[i], list(o[:k]), ospec, cp, num_obs=K, dt=DT)
        st[i] = r["status"]
        if r["u"] is not None:
            u[i] = r["u"]
        h[i, :k] = r["h"][:k]
        if not margins:
            continue
        lo, hi = ocbf.input_bounds(m, ospec)
        Gb, cb = oqp.box_rows(lo, hi)
        mg[i] = oqp.feasibility_margin(np.vstack([r["A"], Gb]), np.concatenate([r["b"], cb]))
    return u, st, h, mg


# (model, K, shared) -> seed; see the module docstring
SOLVE_SEEDS = {
    ('DynamicUnicycle2D', 5, False): 1000,   # 5 infeasible
    ('DynamicUnicycle2D', 5, True): 1000,   # 4 infeasible
    ('DynamicUnicycle2D', 16, False): 1000,   # 7 infeasible
    ('DynamicUnicycle2D', 16, True): 1000,   # 4 infeasible
    ('KinematicBicycle2D', 5, False): 1000,   # 1 infeasible
    ('KinematicBicycle2D', 5, True): 1002,   # 1 infeasible
    ('KinematicBicycle2D', 16, False): 1000,   # 6 infeasible
    ('KinematicBicycle2D', 16, True): 1000,   # 2 infeasible
    ('KinematicBicycle2D_C3BF', 5, False): 1000,   # 8 infeasible
    ('KinematicBicycle2D_C3BF', 5, True): 1000,   # 1 infeasible
    ('KinematicBicycle2D_C3BF', 16, False): 1000,   # 25 infeasible
    ('KinematicBicycle2D_C3BF', 16, True): 1000,   # 6 infeasible
    ('KinematicBicycle2D_DPCBF', 5, False): 1000,   # 6 infeasible
    ('KinematicBicycle2D_DPCBF', 5, True): 1000,   # 2 infeasible
    ('KinematicBicycle2D_DPCBF', 16, False): 1000,   # 13 infeasible
    ('KinematicBicycle2D_DPCBF', 16, True): 1000,   # 4 infeasible
    ('Unicycle2D', 5, False): 1001,   # 2 infeasible
    ('Unicycle2D', 5, True): 1000,   # 1 infeasible
    ('Unicycle2D', 16, False): 1000,   # 4 infeasible
    ('Unicycle2D', 16, True): 1000,   # 2 infeasible
    ('SingleIntegrator2D', 5, False): 1000,   # 2 infeasible
    ('SingleIntegrator2D', 5, True): 1000,   # 2 infeasible
    ('SingleIntegrator2D', 16, False): 1000,   # 4 infeasible
    ('SingleIntegrator2D', 16, True): 1000,   # 1 infeasible
    ('DoubleIntegrator2D', 5, False): 1000,   # 2 infeasible
    ('DoubleIntegrator2D', 5, True): 1000,   # 2 infeasible
    ('DoubleIntegrator2D', 16, False): 1000,   # 11 infeasible
    ('DoubleIntegrator2D', 16, True): 1000,   # 2 infeasible
    # K = 4 (the KMAX = 4 kernel) and K = 20 (f32 rows per agent: 66 560 B of LDS, above the 64 KiB a kernel gets unasked)
    ('DynamicUnicycle2D', 4, False): 1000, ('DynamicUnicycle2D', 4, True): 1000,
    ('DynamicUnicycle2D', 20, False): 1000, ('DynamicUnicycle2D', 20, True): 1000,
    ('KinematicBicycle2D', 4, False): 1000, ('KinematicBicycle2D', 4, True): 1003,
    ('KinematicBicycle2D', 20, False): 1000, ('KinematicBicycle2D', 20, True): 1000,
    ('KinematicBicycle2D_C3BF', 4, False): 1000, ('KinematicBicycle2D_C3BF', 4, True): 1000,
    ('KinematicBicycle2D_C3BF', 20, False): 1000, ('KinematicBicycle2D_C3BF', 20, True): 1000,
    ('KinematicBicycle2D_DPCBF', 4, False): 1000, ('KinematicBicycle2D_DPCBF', 4, True): 1000,
    ('KinematicBicycle2D_DPCBF', 20, False): 1000, ('KinematicBicycle2D_DPCBF', 20, True): 1000,
    ('Unicycle2D', 4, False): 1000, ('Unicycle2D', 4, True): 1000, ('Unicycle2D', 20, False): 1000, ('Unicycle2D', 20, True): 1000,
    ('SingleIntegrator2D', 4, False): 1000, ('SingleIntegrator2D', 4, True): 1000,
    ('SingleIntegrator2D', 20, False): 1000, ('SingleIntegrator2D', 20, True): 1000,
    ('DoubleIntegrator2D', 4, False): 1000, ('DoubleIntegrator2D', 4, True): 1000,
    ('DoubleIntegrator2D', 20, False): 1000, ('DoubleIntegrator2D', 20, True): 1000,
}


# ---- closed loop ---------------------------------------------------------------------------------------------------------
def six_circle_scene():
    """A 6-circle scene for the models other than DynamicUnicycle2D (their loops are checked on a smaller table)."""
    o = np.zeros((6, 7))
    o[:, 0:3] = [[3.0, 3.0, 0.5], [6.0, 8.0, 0.6], [9.0, 4.0, 0.4], [4.5, 11.0, 0.5], [11.0, 10.0, 0.6], [7.5, 1.5, 0.3]]
    return o


def loop_case(name, obs, B, seed, moving=False):
    """B agents with their own specs, start poses clear of the obstacles (but see the end) and 1-3 waypoints each."""
    rng = np.random.default_rng(seed)
    specs = draw_agent_specs(name, B, rng)
    m = model_id(name)
    obs = np.array(obs, dtype=np.float64)
    if moving:
        obs[:, 3:5] = rng.uniform(-0.3, 0.3, (len(obs), 2))
    X0, wl = [], []
    while len(X0) < B:
        p = rng.uniform(0.5, 13.5, 2)
        if len(obs) and np.min(np.hypot(obs[:, 0] - p[0], obs[:, 1] - p[1]) - obs[:, 2]) < 0.7:
            continue
        if m == R.MODEL_SI:
            X0.append([p[0], p[1], rng.uniform(-np.pi, np.pi)])                 # [x, y, yaw]
        elif m == R.MODEL_DI:
            X0.append([p[0], p[1], rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(-np.pi, np.pi)])
        else:
            v0 = rng.uniform(0.2, 1.0) if name in KB_FAMILY else rng.uniform(0.0, 0.8)
            X0.append([p[0], p[1], rng.uniform(-np.pi, np.pi), v0])
        wl.append(rng.uniform(1.0, 13.0, (int(rng.integers(1, 4)), 2)))
    if B >= 33 and len(obs):
        # the last agent of a full-size case starts inside the first obstacle: -2 at its first step without having moved
        # (tracking.py:627-634), a path the relative-degree-1 models hardly reach otherwise
        ang = rng.uniform(-np.pi, np.pi)
        X0[-1][0:2] = obs[0, 0:2] + 0.5 * obs[0, 2] * np.array([np.cos(ang), np.sin(ang)])
    return dict(name=name, specs=specs, X0=np.array(X0), wl=wl, obs=obs, moving=moving)


def oracle_loop(case, T, num_constraints=10, shift=0.0, solve_fn=None):
    """One TrackingOracle per agent.  Returns per agent ``(X [n,4] after each of its n steps, last return code, n, final state
    machine name, final goal index)``; ``shift`` moves every start state (the tie check of the module docstring); ``solve_fn``
    stands in for the CBF-QP (TrackingOracle: the position controller of the select / solve / apply loop)."""
    out = []
    m = model_id(case["name"])
    integ = m in (R.MODEL_SI, R.MODEL_DI)
    for i, spec in enumerate(case["specs"]):
        _, ospec, cp = oracle_args(spec)
        x0 = np.array(case["X0"][i], dtype=np.float64) + shift
        nst = 2 if m == R.MODEL_SI else 4
        yaw0 = x0[nst] if integ else None
        xs = np.concatenate([x0[:nst], np.zeros(4 - nst)]) if integ else x0
        t = tracking.TrackingOracle(m, xs, ospec, dt=DT, obs=case["obs"], num_constraints=num_constraints,
                                    enable_rotation=not integ, dyn_obs=case["moving"], cbf_param=cp, yaw0=yaw0, solve_fn=solve_fn)
        t.set_waypoints(case["wl"][i])
        Xs, ret = [], 0
        for _ in range(T):
            ret = t.control_step()
            Xs.append(t.X.copy())
            if ret != 0:
                break
        out.append((np.array(Xs), ret, len(Xs), t.state_machine, t.current_goal_index))
    return out


# ---- every kernel the rollout's dispatch can select (test_every_kernel_of_the_rollout_dispatch) -----------------------------
RUNG_B, RUNG_T = 65, 10            # one full wave and one lane; a partial last block of the 8- and 16-lane cooperative kernels
BIG_M, BIG_B, BIG_T = 1171, 3, 2   # 1171 rows x 56 B = 65 576 B of LDS: the first table above the 64 KiB a kernel gets unasked


def rung_case(name, per_agent, big=False):
    """``RUNG_B`` agents on the first three circles of the six-circle scene, or (``big``) ``BIG_B`` agents on that scene followed
    by 1165 small circles 500 m away.  Start states, waypoints and table are rounded to f32, so both storage types see the same
    numbers and share one oracle run.  Without ``per_agent`` every agent carries the first agent's spec (the scalar entry point)."""
    if big:
        obs = np.zeros((BIG_M, 7))
        obs[:6] = six_circle_scene()
        obs[6:, 0] = 500.0 + np.arange(BIG_M - 6)
        obs[6:, 1] = 500.0
        obs[6:, 2] = 0.25
    else:
        obs = six_circle_scene()[:3]
    case = loop_case(name, obs, BIG_B if big else RUNG_B, RUNG_SEEDS[name])
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    case["X0"], case["wl"], case["obs"] = f32(case["X0"]), [f32(w) for w in case["wl"]], f32(case["obs"])
    if not per_agent:
        case["specs"] = [dict(case["specs"][0]) for _ in case["specs"]]
    return case


# name -> seed of rung_case, chosen like LOOP_SEEDS: no agent's return code or finishing step moves with the start states
RUNG_SEEDS = {name: 4000 for name in SOLVE_MODELS}

# name -> seed of its closed-loop case; see the module docstring
LOOP_SEEDS = {name: 2000 for name in SOLVE_MODELS}     # the first candidate passed for every model
DYN_SEED = 3000                                        # test_moving_table_against_the_oracle: same tie check, 50 steps


def _du14():
    g = np.load(os.path.join(ROOT, "tests", "golden", "closed_loop.npz"))
    return g["du14/obs"]


def loop_setup(name):
    """``(obstacle table, B, T)`` of the closed-loop case of ``name``."""
    if name == "DynamicUnicycle2D":
        return _du14(), 70, 200
    return six_circle_scene(), 33, 120


def _choose_solve():
    for name in SOLVE_MODELS:
        for K in (4, 5, 16, 20):
            for shared in (False, True):
                for seed in range(1000, 1400):
                    c = solve_case(name, K, shared, seed)
                    u, st, h, mg = oracle_solve(c, margins=True)
                    if (st == 0).any() and (st == 1).any() and set(st) <= {0, 1} and np.abs(mg).min() > 1e-4:
                        print(f"    ({name!r}, {K}, {shared}): {seed},   # {int((st == 1).sum())} infeasible", flush=True)
                        break
                else:
                    print("no seed for", name, K, shared)


def _choose_loop(names):
    for name in names:
        obs, B, T = loop_setup(name)
        for seed in range(2000, 2200):
            c = loop_case(name, obs, B, seed)
            base = [(r[1], r[2]) for r in oracle_loop(c, T)]
            codes = {b[0] for b in base}
            if codes != {0, -1, -2}:
                continue
            if all([(r[1], r[2]) for r in oracle_loop(c, T, shift=s)] == base for s in (1e-12, -1e-12)):
                print(f"    {name!r}: {seed},   # return codes {sorted(b[0] for b in base)}", flush=True)
                break
        else:
            print("no loop seed for", name)


def _choose_rung(names):
    for name in names:
        for seed in range(4000, 4200):
            RUNG_SEEDS[name] = seed
            ok = True
            for per_agent in (True, False):
                for big, T, ncs in ((False, RUNG_T, (8,)), (True, BIG_T, (8, 9))):
                    for nc in ncs:
                        c = rung_case(name, per_agent, big)
                        base = [(r[1], r[2]) for r in oracle_loop(c, T, nc)]
                        ok = ok and all([(r[1], r[2]) for r in oracle_loop(c, T, nc, shift=s)] == base for s in (1e-12, -1e-12))
            if ok:
                print(f"    {name!r}: {seed},", flush=True)
                break
        else:
            print("no rung seed for", name)


def _choose_dyn():
    for seed in range(3000, 3200):
        c = loop_case("KinematicBicycle2D_C3BF", six_circle_scene(), 40, seed, moving=True)
        base = [(r[1], r[2]) for r in oracle_loop(c, 50)]
        if all([(r[1], r[2]) for r in oracle_loop(c, 50, shift=s)] == base for s in (1e-12, -1e-12)) and len({b[0] for b in base}) > 1:
            print("DYN_SEED =", seed, sorted(b[0] for b in base))
            break


if __name__ == "__main__":                       # python tests/_agent_params_cases.py [solve | dyn | <model name> ...]
    what = sys.argv[1:] or ["solve", "dyn"] + list(SOLVE_MODELS)
    if "solve" in what:
        _choose_solve()
    if "dyn" in what:
        _choose_dyn()
    _choose_loop([w for w in what if w in SOLVE_MODELS])
    if "rung" in what:
        _choose_rung(SOLVE_MODELS)
