#!/usr/bin/env python3
"""Golden vectors for the Gatekeeper and MPS shields on the drift-car scenario, from the reference's own code.

Run ONLY in the build container (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_drift_shield.py [--calls-only]

Executed verbatim from the reference (imported through tests/golden/_ref_import.py): ``Gatekeeper``, ``MPS``, ``DriftingCar``,
``DriftingCarSimulator``, ``DriftingEnv``, ``LaneChangeController`` and ``StoppingController``, composed as
examples/drift_car/test_drift.py composes them (:209-373) with its configuration dataclasses and its four test cases, and
run through its loop (:404-523).

What is NOT the example's: ``MPCC`` needs do-mpc and casadi, which are not installed, so the nominal trajectory is a lane
keeper -- a ``LaneChangeController`` aimed at the ego lane, rolled out with ``car.step`` for int(6.0 / dt) steps -- handed
over through ``set_nominal_trajectory`` in the shape the example hands MPCC's prediction over in.  The fixture therefore pins
the shield, not MPCC, and the example's ``get_expected_collision`` table does not carry over.

Writes tests/golden/drift_shield.npz:
  loop_<algo>_<backup>_<case>_*   the 16 closed loops: per step the state, friction, moving-obstacle positions, returned
           input, is_using_backup(), actual_nominal_steps, current_time_idx, next_event_time, len(committed_u_traj); the
           outcome (1 end of track, -2 collision, 0 time-out) and its step; ``stable``: a second run from a start moved by
           1e-12 took the same decisions at every step
  calls_*  single calls from fresh shields at drawn states, with the nominal and the committed trajectory; some with static
           obstacle cars (sobs rows x, y, radius), one to eight moving ones (mobs rows x, y, vx, vy, length, width, radius)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import _ref_import  # noqa: E402

_ref_import.install()
try:                                                          # gatekeeper.py imports solve_ivp and never calls it
    import scipy.integrate  # noqa: F401
except ImportError:
    _si = type(sys)("scipy.integrate")
    _si.solve_ivp = None
    sys.modules.setdefault("scipy", type(sys)("scipy")).integrate = _si
    sys.modules["scipy.integrate"] = _si

sys.path.insert(0, os.path.join(_ref_import.REFERENCE_ROOT, "examples", "drift_car"))
import test_drift as TD  # noqa: E402  (configuration classes, test cases, the reference classes it imports)

CASES = {"high_friction": TD.create_high_friction_test, "middle_lane_only": TD.create_middle_lane_only_test,
         "low_friction": TD.create_low_friction_test, "puddle_surprise": TD.create_puddle_surprise_test}
ALGOS = ("gatekeeper", "mps")
BACKUPS = ("lane_change", "stop")
NOMINAL_TIME = 6.0


def build(algo, backup, case, x0_shift=0.0):
    """setup_environment / setup_vehicle / setup_obstacles_and_puddles / setup_controllers without a figure and without MPCC."""
    cfg = CASES[case]()
    cfg.algo_type, cfg.backup_type = algo, backup
    tr, sim = cfg.track, cfg.simulation
    env = TD.DriftingEnv(track_type=tr.track_type, track_width=tr.lane_width * tr.num_lanes, track_length=tr.track_length,
                         num_lanes=tr.num_lanes)
    ego_y, backup_y = env.get_lane_center(tr.ego_lane_idx), env.get_lane_center(tr.backup_lane_idx)
    X0 = np.array([1.0 + x0_shift, ego_y + x0_shift, np.deg2rad(0), 0, 0, sim.initial_velocity + x0_shift, 0, 0])   # x, y and V moved
    spec = cfg.vehicle.to_dict()
    spec["v_ref"], spec["safety_margin"] = sim.target_velocity, sim.safety_margin
    car = TD.DriftingCar(X0, spec, sim.dt, None)
    TD.setup_obstacles_and_puddles(cfg, env)
    if backup == "stop":
        bc, target = TD.StoppingController(car.robot_spec, sim.dt), None
    else:
        bc, target = TD.LaneChangeController(car.robot_spec, sim.dt, direction="left"), backup_y
    if algo == "mps":
        sh = TD.MPS(robot=car, robot_spec=car.robot_spec, dt=sim.dt, backup_horizon=sim.backup_horizon_time,
                    event_offset=sim.event_offset, ax=None, safety_margin=sim.safety_margin)
    else:
        sh = TD.Gatekeeper(robot=car, robot_spec=car.robot_spec, dt=sim.dt, backup_horizon=sim.backup_horizon_time,
                           event_offset=sim.event_offset, ax=None, nominal_horizon=sim.nominal_horizon_time,
                           safety_margin=sim.safety_margin)
    sh.set_backup_controller(bc, target=target)
    sh.set_environment(env)
    if env.dynamic_obstacles:
        sh.set_moving_obstacles(lambda t=0.0: env.get_dynamic_obstacle_states(t))
    keeper = TD.LaneChangeController(car.robot_spec, sim.dt, direction="left")
    M = int(NOMINAL_TIME / sim.dt)

    def rollout_nominal(state):
        xs, us = [np.array(state, dtype=float).flatten()], []
        cur = np.array(state, dtype=float).reshape(-1, 1)
        for _ in range(M):
            u = keeper.compute_control(cur, ego_y)
            cur = car.step(cur, u)
            xs.append(cur.flatten())
            us.append(np.asarray(u, dtype=float).flatten())
        return np.array(xs), np.array(us)

    return cfg, env, car, sh, rollout_nominal


def record(sh):
    return dict(using_backup=bool(sh.is_using_backup()), ans=int(sh.actual_nominal_steps), idx=int(sh.current_time_idx),
                net=float(sh.next_event_time), clen=int(len(sh.committed_u_traj)))


def mobs_table(env):
    return np.array([[o["x"], o["y"], o["vx"], o["vy"], o["spec"].get("body_length", 4.5), o["spec"].get("body_width", 2.0),
                      o["spec"].get("radius", 1.0)] for o in env.dynamic_obstacles]).reshape(-1, 7)


def run_loop(algo, backup, case, x0_shift=0.0):
    cfg, env, car, sh, rollout_nominal = build(algo, backup, case, x0_shift)
    sim = cfg.simulation
    mu0 = cfg.vehicle.to_dict()["mu"]
    simulator = TD.DriftingCarSimulator(car, env, show_animation=False)
    table0 = mobs_table(env)
    rows, outcome, out_step = [], 0, -1
    for step in range(int(sim.tf / sim.dt)):                  # test_drift.py:433-510
        state, pos = car.get_state(), car.get_position()
        cur = env.get_friction_at_position(pos, default_friction=mu0)
        if abs(cur - car.get_friction()) > 0.01:
            car.set_friction(cur)
        nx, nu = rollout_nominal(state)
        sh.set_nominal_trajectory(nx, nu)
        mob = np.array([[o["x"], o["y"]] for o in env.dynamic_obstacles]).reshape(-1, 2)
        U = sh.solve_control_problem(state, friction=car.get_friction())
        r = record(sh)
        r.update(X=state.flatten().copy(), friction=float(car.get_friction()), mobs=mob, U=np.asarray(U, dtype=float).flatten().copy())
        rows.append(r)
        result = simulator.step(U)
        if result["collision"]:
            outcome, out_step = -2, step
            break
        if pos[0] > env.track_length - 10:
            outcome, out_step = 1, step
            break
    out = {k: np.array([r[k] for r in rows]) for k in rows[0]}
    out["outcome"], out["outcome_step"] = np.int64(outcome), np.int64(out_step)
    out["mobs0"], out["mu0"] = table0, np.float64(mu0)
    out["puddles"] = np.array([[p["x"], p["y"], p["radius"], p["friction"]] for p in env.puddles]).reshape(-1, 4)
    return out


def run_calls(n, seed):
    """Fresh shields at drawn states: the car somewhere behind or beside the case's obstacles at a drawn time.  Every third
    call has one or two static obstacle cars (env.add_obstacle_car: the circle branch of _is_collision), every eighth has the
    moving obstacles filled up to eight; the one-obstacle case gives a moving table of one row."""
    rng = np.random.default_rng(seed)
    rng2 = np.random.default_rng(seed + 1)                        # the extra obstacles, drawn apart so the other draws stay as they were
    rec = {k: [] for k in ("algo", "backup", "X", "friction", "mobs", "sobs", "U", "using_backup", "ans", "idx", "net", "clen", "nx", "nu", "cb")}
    for i in range(n):
        algo, backup = ALGOS[i % 2], BACKUPS[(i // 2) % 2]
        cfg, env, car, sh, rollout_nominal = build(algo, backup, ("high_friction", "low_friction", "middle_lane_only")[(i // 4) % 3])
        t = rng.uniform(0.0, 8.0)
        for o in env.dynamic_obstacles:
            o["x"] += o["vx"] * t + rng.uniform(-3, 3)
        x = np.array([1.0 + 9.0 * t + rng.uniform(-4, 4), 4.0 + rng.uniform(-1.5, 0.8), rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05),
                      rng.uniform(-0.01, 0.01), rng.uniform(5.0, 12.0), rng.uniform(-0.03, 0.03), rng.uniform(-500.0, 500.0)])
        spec1 = lambda r: {"body_length": 4.5, "body_width": 2.0, "a": 1.4, "b": 1.4, "radius": r}
        if i % 3 == 1:
            for j in range(1 + (i // 3) % 2):
                env.add_obstacle_car(x=x[0] + rng2.uniform(12, 70), y=(-4.0, 4.0, 0.0)[(i // 3 + j) % 3] + rng2.uniform(-0.6, 0.6), theta=0.0,
                                     robot_spec=spec1((1.0, 2.5)[j]))
        if i % 8 == 5:
            while len(env.dynamic_obstacles) < 8:
                env.add_moving_obstacle_car(x=x[0] + rng2.uniform(15, 90), y=(-8.0, -4.0, 0.0, 8.0)[len(env.dynamic_obstacles) % 4],
                                            theta=0.0, vx=rng2.uniform(0.0, 6.0), vy=0.0, robot_spec=spec1(1.0))
        nx, nu = rollout_nominal(x)
        sh.set_nominal_trajectory(nx, nu)
        u = sh.solve_control_problem(x.reshape(-1, 1), friction=car.get_friction())
        r = record(sh)
        cx, cu = sh.get_committed_trajectory()
        s = r["ans"]
        assert np.array_equal(cx[:s + 1], nx[:s + 1])             # so only the part from the switching state on is stored
        assert np.array_equal(cu[:s], nu[:s])
        for k, v in r.items():
            rec[k].append(v)
        for k, v in (("algo", i % 2), ("backup", (i // 2) % 2), ("X", x), ("friction", float(car.get_friction())),
                     ("mobs", np.vstack([mobs_table(env), np.full((8, 7), np.nan)])[:8]),                # NaN rows: no such obstacle
                     ("sobs", np.vstack([np.array([[o["x"], o["y"], o["spec"].get("radius", 2.5)] for o in env.obstacles]).reshape(-1, 3),
                                         np.full((2, 3), np.nan)])[:2]),
                     ("U", np.asarray(u, dtype=float).flatten()), ("nx", nx), ("nu", nu),
                     ("cb", np.hstack([cx[s:], np.vstack([cu[s:], np.full((1, 2), np.nan)])]))):   # committed from the switch on: [nb+1, 8 + 2]
            rec[k].append(v)
    out = {k: np.array(v) for k, v in rec.items()}
    print("calls: s =", out["ans"].tolist(), " static:", (~np.isnan(out["sobs"][:, :, 0])).sum(axis=1).tolist(),
          " moving:", (~np.isnan(out["mobs"][:, :, 0])).sum(axis=1).tolist())
    return out


def gen(calls_only=False):
    out = {}
    path = os.path.join(HERE, "drift_shield.npz")
    if calls_only:                                                # --calls-only: keep the loops of the file, rewrite the single calls
        old = np.load(path)
        out = {k: old[k] for k in old.files if k.startswith("loop_")}
    for algo in () if calls_only else ALGOS:
        for backup in BACKUPS:
            for case in CASES:
                a = run_loop(algo, backup, case)
                b = run_loop(algo, backup, case, 1e-12)
                n = min(len(a["U"]), len(b["U"]))
                same = len(a["U"]) == len(b["U"]) and int(a["outcome"]) == int(b["outcome"])
                flips = sum(int(np.any(a[k][:n] != b[k][:n])) for k in ("ans", "idx", "clen", "using_backup"))
                nflip = int(np.sum((a["ans"][:n] != b["ans"][:n]) | (a["idx"][:n] != b["idx"][:n]) | (a["clen"][:n] != b["clen"][:n])
                                   | (a["using_backup"][:n] != b["using_backup"][:n])))
                a["stable"] = np.bool_(same and flips == 0)
                a["flipped_steps"] = np.int64(nflip)
                print(f"{algo:10s} {backup:11s} {case:16s} steps {len(a['U']):4d} outcome {int(a['outcome']):2d} at {int(a['outcome_step']):4d}"
                      f"  backup steps {int(a['using_backup'].sum()):4d}  stable {bool(a['stable'])} ({nflip} steps differ,"
                      f" max |dU| {np.abs(a['U'][:n] - b['U'][:n]).max():.3g})", flush=True)
                for k, v in a.items():
                    out[f"loop_{algo}_{backup}_{case}_{k}"] = v
    for k, a in run_calls(24, 20261016).items():
        out[f"calls_{k}"] = a
    np.savez_compressed(path, **out)
    print("wrote drift_shield.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    gen("--calls-only" in sys.argv[1:])
