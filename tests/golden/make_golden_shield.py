#!/usr/bin/env python3
"""Golden vectors for the Gatekeeper and MPS shields on the evade scenario, from the reference's own code.

Run ONLY in the build container (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_shield.py

Executed verbatim from the reference (imported through tests/golden/_ref_import.py): ``Gatekeeper`` (shielding/gatekeeper.py)
and ``MPS`` (shielding/mps.py) in external-trajectory mode, on the setup of examples/evade/test_evade.py --algo gatekeeper /
--algo mps: ``EvadeEnv`` (envs/evade_env.py), ``DoubleIntegrator2D``, ``EvadeBackupController`` and the example's nominal
controller rolled out with ``dynamics.step`` (test_evade.py:387-408), the bullet predicted by ``get_obstacles(t)`` (:373-384).

Writes tests/golden/shield.npz:
  loops    the example's closed loop (test_evade.py:434-497) for each algorithm and variant: state, bullet_x, u per step,
           is_using_backup(), actual_nominal_steps, current_time_idx, next_event_time, len(committed_u_traj) after the call,
           outcome (1 goal, -2 collision, 0 time-out) and the step it was reached at
  calls    single calls from fresh shields at drawn (state, bullet) pairs: the same fields plus the committed trajectory.

and tests/golden/shield_b.npz, the same keys at scenario "B" of tests/_evade_scenarios.py (no two parameters equal): the
same objects built the same way from B's numbers, the gains set on the EvadeBackupController instance; one loop (variant
"base", LOOP_B) and 20 single calls per algorithm, plus the gains."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.dirname(HERE))

import _evade_scenarios as SC  # noqa: E402
import _ref_import  # noqa: E402

_ref_import.install()
try:                                                          # gatekeeper.py imports solve_ivp and never calls it
    import scipy.integrate  # noqa: F401
except ImportError:
    _si = type(sys)("scipy.integrate")
    _si.solve_ivp = None
    sys.modules.setdefault("scipy", type(sys)("scipy")).integrate = _si
    sys.modules["scipy.integrate"] = _si

from safe_control.envs.evade_env import EvadeEnv  # noqa: E402
from safe_control.robots.double_integrator2D import DoubleIntegrator2D  # noqa: E402
from safe_control.position_control.backup_controller import EvadeBackupController  # noqa: E402
from safe_control.shielding.gatekeeper import Gatekeeper  # noqa: E402
from safe_control.shielding.mps import MPS  # noqa: E402

sys.path.insert(0, os.path.join(_ref_import.REFERENCE_ROOT, "examples", "evade"))
import test_evade as EV  # noqa: E402  (configuration classes + the nominal controller)

# name -> (dt, backup_horizon, nominal_horizon, event_offset); the first is the example's own setting
VARIANTS = {
    "base": (0.1, 12.0, 10.0, 0.05),
    "eo05": (0.1, 12.0, 10.0, 0.5),      # the commitment is followed for several steps between events
    "bh2": (0.1, 2.0, 10.0, 0.05),       # short backup: the index runs past the committed inputs (direct backup fallback)
    "nh3": (0.1, 12.0, 3.0, 0.05),       # 30 nominal steps, 8 candidates
    "dt005": (0.05, 12.0, 10.0, 0.05),
}
ALGOS = ("gatekeeper", "mps")
# scenario B: its parameter set, and the start, bullet position and number of steps of its one loop per algorithm
VARIANTS_B = {"base": (SC.DT["B"], SC.HORIZON["B"], 10.0, 0.05)}
LOOP_B = ((22.0, 0.0, 0.0, 0.0), SC.ENV_KW["B"]["bullet_start_x"], 260)


def build(algo, dt, backup_horizon, nominal_horizon, event_offset, scenario="default"):
    cfg = EV.TestConfig(algo_type=algo)
    s = cfg.simulation
    s.dt, s.backup_horizon_time, s.nominal_horizon_time, s.event_offset = dt, backup_horizon, nominal_horizon, event_offset
    e = cfg.env
    if scenario != "default":                                 # the example's configuration objects with the scenario's numbers
        for k, v in SC.ENV_KW[scenario].items():
            if hasattr(e, k):
                setattr(e, k, v)
        cfg.robot.radius, cfg.robot.a_max, cfg.robot.v_max = (SC.ROBOT[scenario][k] for k in ("radius", "a_max", "v_max"))
        s.safety_margin = SC.ROBOT[scenario]["safety_margin"]
    env = EvadeEnv(hallway_length=e.hallway_length, hallway_width=e.hallway_width, pocket_x=e.pocket_x,
                   pocket_length=e.pocket_length, pocket_width=e.pocket_width, goal_length=e.goal_length,
                   bullet_speed=e.bullet_speed, bullet_length=e.bullet_length, bullet_start_x=e.bullet_start_x,
                   bullet_width=SC.ENV_KW[scenario]["bullet_width"])
    env._draw_bullet_bill = lambda: None                      # no figure
    spec = cfg.robot.to_dict()
    spec["safety_margin"] = s.safety_margin
    goal_bounds = {"x_min": env.goal_x_min, "x_max": env.goal_x_max, "y_min": -env.half_width, "y_max": env.half_width}
    nominal = EV.EvadeNominalController(spec)
    backup = EvadeBackupController(spec, dt, env.get_pocket_center(), env.get_pocket_bounds(), goal_bounds)
    if scenario != "default":
        backup.Kp, backup.Kd = SC.GAINS[scenario]["kp"], SC.GAINS[scenario]["kd"]
    dyn = DoubleIntegrator2D(dt, spec)
    if algo == "mps":                                         # test_evade.py:335-366
        sh = MPS(robot=dyn, robot_spec=spec, dt=dt, backup_horizon=backup_horizon, event_offset=event_offset, ax=None,
                 safety_margin=s.safety_margin)
    else:
        sh = Gatekeeper(robot=dyn, robot_spec=spec, dt=dt, backup_horizon=backup_horizon, nominal_horizon=nominal_horizon,
                        event_offset=event_offset, ax=None, safety_margin=s.safety_margin)
    sh.set_backup_controller(backup)
    sh.set_environment(env)

    def get_obstacles(t=0.0):                                 # test_evade.py:373-384
        b = env.get_bullet_state()
        if not b["active"]:
            return None
        f = b.copy()
        f["x"] = b["x"] + b["vx"] * t
        return f

    sh.set_moving_obstacles(get_obstacles)

    def rollout_nominal(start_state, horizon_time):           # test_evade.py:387-408
        steps = int(horizon_time / dt)
        x_traj = [start_state.flatten()]
        u_traj = []
        curr = start_state.reshape(-1, 1)
        for _ in range(steps):
            u = nominal.compute_control(curr)
            nxt = dyn.step(curr, u)
            x_traj.append(nxt.flatten())
            u_traj.append(u.flatten())
            curr = nxt
        return np.array(x_traj), np.array(u_traj)

    return cfg, env, sh, dyn, rollout_nominal


def record(sh):
    return dict(using_backup=bool(sh.is_using_backup()), ans=int(sh.actual_nominal_steps), idx=int(sh.current_time_idx),
                net=float(sh.next_event_time), clen=int(len(sh.committed_u_traj)))


def run_loop(algo, variant, scenario="default"):
    dt, bh, nh, eo = (VARIANTS if scenario == "default" else VARIANTS_B)[variant]
    cfg, env, sh, dyn, rollout_nominal = build(algo, dt, bh, nh, eo, scenario)
    state = np.array([cfg.simulation.initial_x, 0.0, 0.0, 0.0]).reshape(-1, 1)
    T = int(cfg.simulation.tf / dt)
    if scenario != "default":
        x0, env.bullet_x, T = LOOP_B
        state = np.array(x0, dtype=float).reshape(-1, 1)
    rows = []
    outcome, out_step = 0, -1
    for step in range(T):                                     # test_evade.py:434-497
        pos = state[:2, 0]
        nom_x, nom_u = rollout_nominal(state, nh)
        sh.set_nominal_trajectory(nom_x, nom_u)
        x_rec, b_rec = state.flatten().copy(), float(env.bullet_x)
        control = sh.solve_control_problem(state)
        r = record(sh)
        r.update(X=x_rec, bullet_x=b_rec, U=np.asarray(control, dtype=float).flatten().copy())
        rows.append(r)
        state = dyn.step(state, control)
        vx, vy = state[2, 0], state[3, 0]
        vm = np.sqrt(vx ** 2 + vy ** 2)
        if vm > cfg.robot.v_max:
            state[2, 0] = vx * cfg.robot.v_max / vm
            state[3, 0] = vy * cfg.robot.v_max / vm
        env.step_bullet(dt)
        if env.check_obstacle_collision(pos, cfg.robot.radius)[0]:
            outcome, out_step = -2, step
            break
        if env.check_goal_reached(pos):
            outcome, out_step = 1, step
            break
    out = {k: np.array([r[k] for r in rows]) for k in rows[0]}
    out["outcome"], out["outcome_step"] = np.int64(outcome), np.int64(out_step)
    out["params"] = np.array([dt, bh, nh, eo])
    print(f"{algo:10s} {variant:6s} steps {len(rows):4d} outcome {outcome:2d} at {out_step:4d}  backup steps {int(out['using_backup'].sum()):4d}"
          f"  calls with s > 0 {int((out['ans'] > 0).sum())}  past the commitment {int((out['idx'] > out['clen']).sum())}")
    return out


def draw(rng, kind):
    """The draws of make_golden_backup.py."""
    if kind == 0:      # hallway, bullet close behind
        x = np.array([rng.uniform(8, 50), rng.uniform(-1.2, 1.2), rng.uniform(0, 1.5), rng.uniform(-0.3, 0.3)])
        bx = x[0] - rng.uniform(4, 14)
    elif kind == 1:    # below the pocket
        x = np.array([rng.uniform(26.5, 33.5), rng.uniform(-1.0, 1.4), rng.uniform(-0.5, 1.0), rng.uniform(-0.3, 0.8)])
        bx = x[0] - rng.uniform(3, 20)
    elif kind == 2:    # inside the pocket
        x = np.array([rng.uniform(26.5, 33.5), rng.uniform(2.8, 5.2), rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4)])
        bx = rng.uniform(0, 60)
    elif kind == 3:    # bullet far away or ahead
        x = np.array([rng.uniform(5, 50), rng.uniform(-1.0, 1.0), rng.uniform(0.5, 1.5), rng.uniform(-0.2, 0.2)])
        bx = x[0] + rng.uniform(6, 20) if rng.uniform() < 0.5 else -10.0
    else:              # near the goal
        x = np.array([rng.uniform(50, 58.5), rng.uniform(-1.0, 1.0), rng.uniform(0.0, 1.5), rng.uniform(-0.2, 0.2)])
        bx = x[0] - rng.uniform(5, 30)
    return x, bx


def run_calls(algo, n, seed, scenario="default"):
    dt, bh, nh, eo = (VARIANTS if scenario == "default" else VARIANTS_B)["base"]
    rng = np.random.default_rng(seed)
    M = int(nh / dt)
    nb = int(bh / dt)
    L = M + 1 + nb
    rec = dict(X=[], bullet_x=[], U=[], using_backup=[], ans=[], idx=[], net=[], clen=[], cx=[], cu=[])
    for i in range(n):
        x, bx = draw(rng, i % 5) if scenario == "default" else SC.draw_call_b(rng, i % 5)
        cfg, env, sh, dyn, rollout_nominal = build(algo, dt, bh, nh, eo, scenario)
        env.bullet_x = float(bx)
        nom_x, nom_u = rollout_nominal(x.reshape(-1, 1), nh)
        sh.set_nominal_trajectory(nom_x, nom_u)
        u = sh.solve_control_problem(x.reshape(-1, 1))
        r = record(sh)
        cx, cu = sh.get_committed_trajectory()
        px = np.full((L, 4), np.nan)
        px[:len(cx)] = cx
        pu = np.full((L - 1, 2), np.nan)
        pu[:len(cu)] = cu
        for k, v in r.items():
            rec[k].append(v)
        rec["X"].append(x)
        rec["bullet_x"].append(bx)
        rec["U"].append(np.asarray(u, dtype=float).flatten())
        rec["cx"].append(px)
        rec["cu"].append(pu)
    out = {k: np.array(v) for k, v in rec.items()}
    print(f"{algo:10s} calls {n}: s = {out['ans'].tolist()}")
    return out


def gen(scenario="default"):
    out = {}
    variants, n_calls, seeds, name = (VARIANTS, 30, (20261016, 20261017), "shield.npz") if scenario == "default" else (
        VARIANTS_B, 20, (20261020, 20261021), "shield_b.npz")
    for algo in ALGOS:
        for v in variants:
            for k, a in run_loop(algo, v, scenario).items():
                out[f"loop_{algo}_{v}_{k}"] = a
        for k, a in run_calls(algo, n_calls, seeds[0] if algo == "gatekeeper" else seeds[1], scenario).items():
            out[f"calls_{algo}_{k}"] = a
    _, env, sh, _, _ = build("gatekeeper", *variants["base"], scenario)
    out["env"] = np.array([env.hallway_length, env.half_width, env.pocket_x_min, env.pocket_x_max, env.pocket_y_min, env.pocket_y_max,
                           env.goal_x_min, env.goal_x_max, env.bullet_speed, env.bullet_length, env.bullet_width, env.bullet_start_x])
    out["spec"] = np.array([sh.robot_spec["radius"], sh.robot_spec["a_max"], sh.robot_spec["v_max"], sh.safety_margin,
                            sh.horizon_discount])
    if scenario != "default":
        out["gains"] = np.array([sh.backup_controller.Kp, sh.backup_controller.Kd])
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print("wrote", name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    gen()
    gen("B")
