"""Scenes for the fused arm rollout (csrc/manip_cbf_qp.hip: manip_rollout_kernel<1..4>) and what oracle.manipulator's
ArmTrackingOracle makes of them.  Host only, seeded; tests/test_manip_rollout_gpu.py runs the kernel on them.

24 arms with their own start angles and two waypoints each (the generator of the fleet test of tests/test_manipulator_gpu.py)
around a shared obstacle table.  The table of a scene is laid out so that the barrier rows change the nominal input on many
arm-steps and the arms end in more than one way; the counts the oracle gives are in SCENES below and are asserted by the test.

The rollout kernel is instantiated by rows per lane, RPL = ceil((min(num_constraints, min(M, num_constraints) 25) + 6) / 64).
"""
import functools
import math

import numpy as np

from oracle import manipulator as M
from oracle import qp as Q

BASE = (5.0, 3.5)
B, T = 24, 120
SPEC = {"w_max": 2.0, "Kp": 5.0, "radius": 0.25, "reached_threshold": 0.4}
SM = {"idle": 0, "track": 1, "stop": 2, "rotate": 3}

# name: (number of obstacles, num_constraints, rows per lane, steps, seed of the layout)
SCENES = {
    "m1": dict(M=1, nc=150, rpl=1, T=120, seed=1),
    "m6": dict(M=6, nc=150, rpl=3, T=120, seed=2),
    "m10": dict(M=10, nc=250, rpl=4, T=120, seed=3),
    "m10cap60": dict(M=10, nc=60, rpl=2, T=120, seed=4),         # the cap cuts the third-nearest obstacle after 10 rows
    "m5rows3": dict(M=5, nc=3, rpl=1, T=120, seed=5),            # 3 rows: the first three circles of link 0 against the nearest obstacle
}


def rpl_of(Mo, nc, circles=25):
    return (min(nc, min(Mo, nc) * circles) + 6 + 63) // 64


def arms(seed=12, n=B):
    """Start angles and waypoint lists of the fleet test."""
    rng = np.random.default_rng(seed)
    q0 = rng.uniform(-1.2, 1.2, (n, 3))
    wl = []
    for _ in range(n):
        ang = rng.uniform(-np.pi, np.pi, 2); rad = rng.uniform(1.6, 3.0, 2)
        wl.append(np.stack([BASE[0] + rad * np.cos(ang), BASE[1] + rad * np.sin(ang)], axis=1))
    return q0, wl


def table(name):
    """Obstacles [M,7] on rings around the base: the nearest one close in (for 'm5rows3' close enough for the first circles of
    link 0 to meet it), the others between 1.7 and 3.5."""
    cfg = SCENES[name]
    rng = np.random.default_rng([31, cfg["seed"]])
    Mo = cfg["M"]
    obs = np.zeros((Mo, 7))
    for r in range(Mo):
        if name == "m5rows3" and r == 0:
            rho, rad = 0.56, 0.2
        else:
            rho, rad = rng.uniform(1.7, 3.5), rng.uniform(0.2, 0.35)
        phi = rng.uniform(-np.pi, np.pi)
        obs[r, :3] = [BASE[0] + rho * math.cos(phi), BASE[1] + rho * math.sin(phi), rad]
    return obs


def oracle_run(q0, wl, obs, nc, steps, alpha=1.0, spec=SPEC, start=None, watch=False):
    """ArmTrackingOracle per arm for `steps` steps.  Returns dict(X [steps,B,3] (frozen after an arm finishes), U [steps,B,3] (the
    last input applied), ret, ret_step, sm, wp, goal [B,3] = (gx, gy, valid), n_changed (arm-steps on which the barrier changed the
    nominal input by more than 1e-6), stop0 (arms that start in 'stop')).  `start`: per-arm dict(waypoints, index, sm, goal) read
    back from a controller, instead of set_waypoints.  `watch`: also `near` [B], the smallest distance of a reached / rotate /
    feasibility decision of the arm to its threshold."""
    n = len(q0)
    X = np.zeros((steps, n, 3)); U = np.zeros((steps, n, 3))
    ret = np.zeros(n, dtype=np.int64); ret_step = np.full(n, -1, dtype=np.int64)
    sm = np.zeros(n, dtype=np.int64); wp = np.zeros(n, dtype=np.int64); goal = np.zeros((n, 3))
    near = np.full(n, np.inf)
    n_changed = stop0 = 0
    for i in range(n):
        o = M.ArmTrackingOracle(q0[i], spec, base=BASE, obs=obs, num_constraints=nc, alpha=alpha)
        if start is None:
            o.set_waypoints(wl[i])
        else:
            s = start[i]
            o.waypoints, o.current_goal_index, o.state_machine = s["waypoints"], int(s["index"]), s["sm"]
            o.goal = None if s["goal"] is None else np.array(s["goal"], dtype=np.float64)
        stop0 += o.state_machine == "stop"
        u_last = np.zeros(3)
        for k in range(steps):
            if ret[i] == 0:
                x_before = o.X.copy()
                if watch and o.current_goal_index < len(o.waypoints):
                    w = o.waypoints[o.current_goal_index]
                    near[i] = min(near[i], abs(np.linalg.norm(M.end_effector(o.X, BASE) - w[:2]) - o.reached_threshold))
                    if o.state_machine == "stop":
                        near[i] = min(near[i], abs(abs(math.atan2(w[1] - o.X[1], w[0] - o.X[0])) - o.rotation_threshold))
                code = o.control_step()
                if watch and len(obs):
                    nr = o.ranked_obstacles()
                    A, b, _ = M.assemble_rows(x_before, list(nr), o.spec, alpha, nc, o.dt, "cbf", BASE)
                    rows = min(nc, len(nr) * 25)
                    G = np.vstack([A[:rows], np.eye(3), -np.eye(3)]); c = np.concatenate([b[:rows], np.full(6, o.spec["w_max"])])
                    near[i] = min(near[i], abs(Q.feasibility_margin(G, c)))
                if code != -2:
                    u_last = o.u_pos.copy()
                    if o.goal is not None:
                        n_changed += int(np.abs(o.u_pos - M.nominal_input(x_before, o.goal, o.spec, BASE)).max() > 1e-6)
                if code != 0:
                    ret[i], ret_step[i] = code, k
            X[k, i], U[k, i] = o.X, u_last
        sm[i], wp[i] = SM[o.state_machine], o.current_goal_index
        if o.goal is not None:
            goal[i] = [o.goal[0], o.goal[1], 1.0]
    return dict(X=X, U=U, ret=ret, ret_step=ret_step, sm=sm, wp=wp, goal=goal, n_changed=n_changed, stop0=stop0, near=near)


@functools.lru_cache(maxsize=None)
def scene(name, alpha=1.0, steps=None):
    """dict(q0, wl, obs, nc, T, oracle) of a scene; the oracle's run is computed once and shared by the tests."""
    cfg = SCENES[name]
    q0, wl = arms()
    obs = table(name)
    steps = cfg["T"] if steps is None else steps
    assert rpl_of(cfg["M"], cfg["nc"]) == cfg["rpl"]
    return dict(q0=q0, wl=wl, obs=obs, nc=cfg["nc"], T=steps, rpl=cfg["rpl"], oracle=oracle_run(q0, wl, obs, cfg["nc"], steps, alpha))
