"""Injected per-agent situations for the two kernels of csrc/tracking_quad.hip (sc_quadtrack_select_batch / sc_quadtrack_apply_batch)
and what oracle/tracking_quad.py's select() / apply(u) make of them.  Host only, seeded; tests/test_quadtrack_cases.py checks the
batches here, tests/test_quadtrack_kernels_gpu.py holds the kernels to them.

An agent is a state, a state machine, a stored goal with its valid flag, a waypoint index, a waypoint list, the return code it
enters with and the input to apply.  Only situations the reference can be in are drawn (index < n_wp in 'track' / 'stop' /
'rotate'; index == n_wp with no goal in 'idle'; one 'stop' in five keeps a stored goal, which set_waypoints never leaves behind but
control_step reads like any other).  One obstacle table of 40 rows is shared by a batch, a launch takes its first M
rows; K, M, enable_rotation and reached_threshold belong to the launch, so a batch is run under several configurations (CONFIGS).

Exact cases -- the only comparisons allowed to sit ON a threshold, because both sides then compute the same number:
  * distance ties: the agents at CENTRE and the rows at CENTRE + (+-0.75, +-1.0) and + (1.25, 0).  Every coordinate is a multiple of
    1/4, the differences, their squares (0.5625, 1, 1.5625) and the sum are exact, the root is 1.25 under hypot, under
    sqrt(dx*dx + dy*dy) and under a fused multiply-add alike.  Rows 2 and 11 share a centre (radii differ): a tie for every agent,
    whatever the arithmetic, since both distances come from the same numbers.
  * reached_threshold: a waypoint at position + (0.5, 0), position on a 1/64 grid: dx = -0.5, dy = 0, distance 0.5 exactly; under
    reached_threshold = 0.5 the test `<` is false on both sides.  And a waypoint at (0.3, y) for an agent at (0, y): dx = -0.3 (the
    double), sqrt(fl(dx*dx)) == 0.3 in IEEE arithmetic; under reached_threshold = 0.3 the test is false on both sides (in f32 storage
    that waypoint is float(0.3), 1.2e-8 away: no longer a tie, and outside the margin).
  * has_stopped: 0.05 is not representable and no speed lands on it exactly: no exact case, every draw keeps its margin.
"""
import functools
import math

import numpy as np

from oracle import tracking_quad as T

MODELS = ("Quad2D", "Quad3D", "VTOL2D")
SM_NAMES = ("idle", "track", "stop", "rotate")
IDLE, TRACK, STOP, ROTATE = range(4)
B_MAIN, W, M_TABLE = 200, 4, 40
SEED = 3
MARGIN = 1e-9
JUNK = 777.0                                     # waypoint rows past n_wp: never to be read
REGION = 20.0                                   # agents, waypoints and table rows lie in [0.5, REGION - 0.5]^2
CENTRE = np.array([10.0, 10.0])
TIE_ROWS = (2, 4, 6, 9, 11)                      # all at distance 1.25 from CENTRE; 2 and 11 share a centre
DT = 0.05
STEP_INDEX = 7                                   # what a launch writes into ret_step for an agent that ends in it
RET_STEP_FROZEN = 3                              # what frozen agents carry there

# K x M: both instantiations of the select kernel (<8>: K <= 8) at both of their edges, tables shorter than, equal to and longer than K
MAIN = (dict(K=9, M=40, enable_rotation=1, reached_threshold=0.3), dict(K=8, M=40, enable_rotation=0, reached_threshold=0.5),
        dict(K=16, M=40, enable_rotation=1, reached_threshold=0.5), dict(K=1, M=40, enable_rotation=0, reached_threshold=0.3))
EDGE = tuple(dict(K=K, M=M, enable_rotation=(i + j) % 2, reached_threshold=(0.3, 0.5)[(i + j // 2) % 2])
             for i, K in enumerate((1, 8, 9, 16)) for j, M in enumerate(sorted({0, 1, K - 1, K})))
CONFIGS = MAIN + EDGE
BIG = dict(K=16, M=1170, enable_rotation=1, reached_threshold=0.3)          # the largest table check_quadtrack accepts


def dims(model):
    """nx, nu, n_pos."""
    return {"Quad2D": (6, 2, 2), "Quad3D": (12, 4, 3), "VTOL2D": (6, 4, 2)}[model]


def u_box(model):
    s = T.default_spec(model)
    if model == "Quad2D":
        return np.full(2, s["f_min"]), np.full(2, s["f_max"])
    if model == "Quad3D":
        return np.full(4, s["u_min"]), np.full(4, s["u_max"])
    return (np.array([s["throttle_min"]] * 3 + [s["elevator_min"]]), np.array([s["throttle_max"]] * 3 + [s["elevator_max"]]))


def _rot(th, px, py):
    """Obstacle frame -> world offset (the inverse of the rotation in the collision test)."""
    return np.array([math.cos(th) * px - math.sin(th) * py, math.sin(th) * px + math.cos(th) * py])


def make_table(rng):
    t = np.zeros((M_TABLE, 7))
    t[0] = [5.0, 5.0, 0.4, 0, 0, 0, 0]
    t[1] = [15.0, 5.0, 0.6, 0.35, 2.0, 0.4, 1]
    t[2] = [CENTRE[0] + 0.75, CENTRE[1] + 1.0, 0.3, 0, 0, 0, 0]
    t[3] = [5.0, 15.0, 0.5, 0.7, 4.0, -0.7, 1]
    t[4] = [CENTRE[0] - 0.75, CENTRE[1] + 1.0, 0.35, 0, 0, 0, 0]
    t[5] = [16.0, 16.0, 0.6, 0.6, 2.5, 0.3, 1]                   # a non-integer exponent: pow of a negative base is NaN, no collision
    t[6] = [CENTRE[0] + 1.25, CENTRE[1], 0.2, 0, 0, 0, 0]
    t[8] = [2.5, 10.5, 0.4, 0.9, 1.5, 0.0, 1]                   # flag 1 with an exponent below 2: a circle of radius 0.4 (tracking.py:440)
    t[9] = [CENTRE[0] - 0.75, CENTRE[1] - 1.0, 0.25, 0, 0, 0, 0]
    t[11] = [CENTRE[0] + 0.75, CENTRE[1] + 1.0, 0.15, 0, 0, 0, 0]
    placed = [0, 1, 2, 3, 4, 5, 6, 8, 9, 11]
    for m in range(M_TABLE):
        if m in placed:
            continue
        while True:
            c = rng.uniform(0.5, REGION - 0.5, 2)
            if np.linalg.norm(c - CENTRE) > 2.6 and min(np.linalg.norm(c - t[j, :2]) for j in placed) > 2.2:
                break
        if m in (7, 10) or rng.random() < 0.65:
            t[m] = [c[0], c[1], rng.uniform(0.15, 0.45), 0, 0, 0, 0]
        else:
            t[m] = [c[0], c[1], rng.uniform(0.3, 0.8), rng.uniform(0.3, 0.8), rng.choice([2.0, 4.0, 2.5]), rng.uniform(-1.5, 1.5), 1]
        placed.append(m)
    return t


def big_table(seed=SEED):
    """BIG['M'] rows around the region of the batch (circles and superellipsoids)."""
    rng = np.random.default_rng([seed, 99])
    n = BIG["M"]
    t = np.zeros((n, 7))
    t[:, :2] = rng.uniform(-30.0, 50.0, (n, 2))
    t[:, 2] = rng.uniform(0.15, 0.45, n)
    se = rng.random(n) < 0.3
    t[se, 3], t[se, 4], t[se, 5], t[se, 6] = rng.uniform(0.3, 0.8, se.sum()), 4.0, rng.uniform(-1.5, 1.5, se.sum()), 1.0
    return t


def is_superell(row):
    return bool(np.isclose(row[6], 1.0) and row[4] >= 2.0)


@functools.lru_cache(maxsize=None)
def cases(model, seed=SEED):
    """The B_MAIN agents of one model, shuffled: dict of arrays X [B,nx], sm, goal [B,4] = (gx, gy, gz, valid), wp_index, n_wp,
    waypoints [B,W,3], ret_in, ret_step_in, u [B,nu], u_last [B,nu]; table [40,7]; placed: name -> agent mask, what an agent was
    BUILT for (what it turned out to do is in tags())."""
    rng = np.random.default_rng([seed, MODELS.index(model)])
    q3, vt = model == "Quad3D", model == "VTOL2D"
    nx, nu, npos = dims(model)
    spec = T.default_spec(model)
    R = spec["radius"]
    table = make_table(rng)
    lo, hi = u_box(model)
    vel = slice(6, 8) if q3 else slice(3, 5)                  # planar velocity
    yaw_i = 5 if q3 else 2
    agents = []

    def base(sm=None, pos=None):
        a = {}
        X = np.zeros(nx)
        X[:2] = rng.uniform([0.5, 1.0 if vt else 0.5], REGION - 0.5) if pos is None else pos
        if q3:
            X[2], X[3:5], X[5] = rng.uniform(0, 3), rng.uniform(-0.5, 0.5, 2), rng.uniform(-3, 3)
            X[6:9], X[9:12] = rng.uniform(-2, 2, 3), rng.uniform(-1, 1, 3)
        elif vt:
            X[2], X[3], X[4], X[5] = rng.uniform(-0.4, 0.4), rng.uniform(3, 12), rng.uniform(-2, 2), rng.uniform(-0.5, 0.5)
        else:
            X[2], X[3:5], X[5] = rng.uniform(-0.6, 0.6), rng.uniform(-2, 2, 2), rng.uniform(-1, 1)
        n = int(rng.integers(1, W + 1))
        wps = np.full((W, 3), JUNK)
        wps[:n, :2] = rng.uniform(0.5, REGION - 0.5, (n, 2))
        wps[:n, 2] = rng.uniform(0, 3, n) if q3 else 0.0
        a["sm"] = int(rng.choice(4, p=[0.12, 0.4, 0.24, 0.24])) if sm is None else sm
        a["X"], a["n_wp"], a["wps"] = X, n, wps
        a["idx"] = n if a["sm"] == IDLE else int(rng.integers(n))
        a["ret_in"] = None                                    # frozen or running: drawn below, where no case needs the agent to run
        u = rng.uniform(lo, hi)
        if rng.random() < 0.3:                                # outside the input box: apply() takes the input as it comes
            u = (lo + hi) / 2 + (u - (lo + hi) / 2) * 1.5
        a["u"], a["u_last"] = u, rng.uniform(lo, hi)
        a["placed"] = set()
        shape(a)
        return a

    def goal_angle(a):
        w = a["wps"][a["idx"]]
        return math.atan2(w[1] - a["X"][1], w[0] - a["X"][0])

    def shape(a):
        """What depends on the state machine the agent enters in."""
        X, sm = a["X"], a["sm"]
        if sm == TRACK and rng.random() < 0.35:               # at its waypoint (below both values of reached_threshold)
            ang = rng.uniform(-math.pi, math.pi)
            a["wps"][a["idx"], :2] = X[:2] + rng.uniform(0.05, 0.25) * np.array([math.cos(ang), math.sin(ang)])
        if sm == STOP:
            c = int(rng.integers(4))
            if c in (0, 1):
                X[vel] *= rng.uniform(0.005, 0.04) / np.linalg.norm(X[vel])
                if q3:
                    X[8] = rng.uniform(-0.01, 0.01)
            if q3 and c in (0, 2):
                X[9:12] *= rng.uniform(0.005, 0.04) / np.linalg.norm(X[9:12])
        if sm in (STOP, ROTATE) and rng.random() < 0.5:       # heading inside rotation_threshold of the bearing of its waypoint
            X[yaw_i] = goal_angle(a) + rng.choice([-1, 1]) * rng.uniform(0.01, 0.09)
        g = np.zeros(4)
        if sm == IDLE:
            g[:npos] = rng.uniform(0.5, 11.5, npos)           # a stale goal, flagged invalid
        elif sm == STOP and rng.random() < 0.8:
            g[:npos] = rng.uniform(0.5, 11.5, npos)           # set_waypoints leaves 'stop' without a goal (tracking.py:224-228)
        else:
            g[:npos], g[3] = a["wps"][a["idx"], :npos], 1.0
        a["goal"] = g

    def add(a, *names):
        a["placed"].update(names)
        agents.append(a)

    circles = [m for m in range(M_TABLE) if not is_superell(table[m]) and m not in TIE_ROWS and m != 8]
    ells = [m for m in range(M_TABLE) if is_superell(table[m]) and table[m, 4] != 2.5]
    # angles within 1e-3 of +-pi, rates towards the wrap (three in four) or away from it
    for k in ((3, 4, 5) if q3 else (2,)):
        for j in range(9):
            a = base(sm=TRACK if j % 2 else None)
            s = 1.0 if j % 6 < 3 else -1.0
            a["X"][k] = s * (math.pi - rng.uniform(1e-4, 1e-3))
            a["X"][k + (6 if q3 else 3)] = s * rng.uniform(0.8, 1.2) * (-1.0 if j % 3 == 2 else 1.0)
            a["ret_in"] = 0
            add(a, f"near_pi_{k}")
    # collisions before the step
    for j in range(8):
        m = (0, 7, 10)[j] if j < 3 else int(rng.choice(circles))
        ang = rng.uniform(-math.pi, math.pi)
        a = base(pos=table[m, :2] + rng.uniform(0.2, 0.8) * (table[m, 2] + R) * np.array([math.cos(ang), math.sin(ang)]))
        a["ret_in"] = 0 if j < 6 else a["ret_in"]
        add(a, "in_circle")
    for j in range(8):
        m = (1, 3, 5)[j] if j < 3 else int(rng.choice(ells))
        sx, sy = (1, 1) if table[m, 4] == 2.5 else rng.choice([-1, 1], 2)
        off = _rot(table[m, 5], sx * rng.uniform(0.1, 0.5) * (table[m, 2] + R), sy * rng.uniform(0.1, 0.5) * (table[m, 3] + R))
        a = base(pos=table[m, :2] + off)
        a["ret_in"] = 0 if j < 6 else a["ret_in"]
        add(a, "in_superell")
    for j in range(3):                                        # inside row 5 by shape, but pow(negative, 2.5) is NaN: no collision
        off = _rot(table[5, 5], -rng.uniform(0.1, 0.4) * (table[5, 2] + R), rng.uniform(0.1, 0.4) * (table[5, 3] + R))
        a = base(pos=table[5, :2] + off)
        a["ret_in"] = 0
        add(a, "in_superell_nan")
    for j in range(3):                                        # row 8: a circle although its flag is 1; as a superellipsoid it would be NaN here
        a = base(pos=table[8, :2] + np.array([-0.5 + 0.05 * j, 0.1]))
        a["ret_in"] = 0
        add(a, "in_flag1_circle")
    # collisions only after the step: just outside, flying in at 3 m/s (0.15 per step)
    for j in range(8):
        m = (0, 7)[j] if j < 2 else int(rng.choice(circles))
        ang = rng.uniform(-math.pi, math.pi)
        d = np.array([math.cos(ang), math.sin(ang)])
        a = base(sm=TRACK, pos=table[m, :2] + (table[m, 2] + R + rng.uniform(0.02, 0.06)) * d)
        a["X"][vel] = -3.0 * d
        a["ret_in"] = 0
        add(a, "towards_circle")
    for j in range(5):
        m = (1, 3)[j] if j < 2 else int(rng.choice(ells))
        s = 1.0 + rng.uniform(0.03, 0.08)                     # on the diagonal of the obstacle frame, 3 .. 8 % outside
        e = table[m, 4]
        off = _rot(table[m, 5], s * 0.5 ** (1 / e) * (table[m, 2] + R), s * 0.5 ** (1 / e) * (table[m, 3] + R))
        a = base(sm=TRACK, pos=table[m, :2] + off)
        a["X"][vel] = -3.0 * off / np.linalg.norm(off)
        a["ret_in"] = 0
        add(a, "towards_superell")
    # exact cases (module docstring)
    for j in range(4):
        a = base(sm=(TRACK, STOP, ROTATE, TRACK)[j], pos=CENTRE.copy())
        if vt:
            a["X"][2] = rng.uniform(-0.3, 0.3)                # rows 2, 6 and 11 inside the cone
        a["ret_in"] = 0
        add(a, "exact_tie")
    for j in range(3):
        a = base(sm=TRACK, pos=rng.integers(64, 1200, 2) / 64.0)
        a["wps"][a["idx"], :2] = a["X"][:2] + np.array([0.5, 0.0])
        a["goal"][:npos], a["goal"][3] = a["wps"][a["idx"], :npos], 1.0
        a["ret_in"] = 0
        add(a, "exact_reached")
    for j in range(3):
        a = base(sm=TRACK, pos=np.array([0.0, rng.integers(64, 1200) / 64.0]))
        a["wps"][a["idx"], :2] = [0.3, a["X"][1]]
        a["goal"][:npos], a["goal"][3] = a["wps"][a["idx"], :npos], 1.0
        a["ret_in"] = 0
        add(a, "exact_reached")
    if vt:
        for j in range(4):
            a = base()
            a["X"][1], a["ret_in"] = -rng.uniform(0.05, 0.5), 0
            add(a, "below_ground")
        for j in range(4):
            a = base(sm=TRACK)
            a["X"][1], a["X"][4], a["ret_in"] = rng.uniform(0.01, 0.04), -rng.uniform(1.5, 3.0), 0
            add(a, "towards_ground")
        for j in range(4):
            a = base()
            a["X"][2], a["ret_in"] = rng.choice([-1, 1]) * rng.uniform(15.2, 17.0), 0     # robot_spec['pitch_max'] is compared as given: 15
            add(a, "past_pitch_limit")
        for j in range(6):                                    # every row behind: outside the table's region, looking away from it
            a = base(pos=np.array([rng.uniform(26, 28), rng.uniform(8, 12)]) if j < 3 else np.array([-rng.uniform(6, 8), rng.uniform(8, 12)]))
            a["X"][2] = rng.uniform(-0.1, 0.1) if j < 3 else rng.choice([-1, 1]) * (math.pi - rng.uniform(0.02, 0.1))
            a["ret_in"] = 0
            add(a, "empty_cone")
    while len(agents) < B_MAIN:
        add(base())
    assert len(agents) == B_MAIN
    free = [a for a in agents if a["ret_in"] is None]
    for j, k in enumerate(rng.permutation(len(free))):        # one agent in eight enters frozen
        free[k]["ret_in"] = int(rng.choice([-1, -2])) if j < B_MAIN // 8 else 0
    order = rng.permutation(B_MAIN)                           # lanes of one wave take different branches: never sorted by kind
    agents = [agents[i] for i in order]
    out = dict(model=model, table=table,
               X=np.array([a["X"] for a in agents]), sm=np.array([a["sm"] for a in agents], dtype=np.int32),
               goal=np.array([a["goal"] for a in agents]), wp_index=np.array([a["idx"] for a in agents], dtype=np.int32),
               n_wp=np.array([a["n_wp"] for a in agents], dtype=np.int32), waypoints=np.array([a["wps"] for a in agents]),
               ret_in=np.array([a["ret_in"] for a in agents], dtype=np.int32), u=np.array([a["u"] for a in agents]),
               u_last=np.array([a["u_last"] for a in agents]))
    out["ret_step_in"] = np.where(out["ret_in"] == 0, -1, RET_STEP_FROZEN).astype(np.int32)
    names = sorted(set().union(*(a["placed"] for a in agents)))
    out["placed"] = {n: np.array([n in a["placed"] for a in agents]) for n in names}
    return out


@functools.lru_cache(maxsize=None)
def shared_cases(model, seed=SEED):
    """The same agents on ONE waypoint list of three (waypoints_shared = 1).  `waypoints` [W,3] and `n_wp_shared` (3) are the launch's;
    `n_wp` stays per agent with entry 0 set to 3: a kernel that reads past entry 0 under waypoints_shared meets other numbers."""
    c = dict(cases(model, seed))
    rng = np.random.default_rng([seed, MODELS.index(model), 1])
    npos = dims(model)[2]
    wps = np.full((W, 3), JUNK)
    wps[:3, :2] = rng.uniform(2.0, REGION - 2.0, (3, 2))
    wps[:3, 2] = rng.uniform(0, 3, 3) if model == "Quad3D" else 0.0
    X = c["X"].copy()
    idx = np.where(c["sm"] == IDLE, 3, c["wp_index"] % 3).astype(np.int32)
    for i in np.flatnonzero((c["sm"] == TRACK) & (np.arange(B_MAIN) % 3 == 0)):     # some of them at their waypoint
        ang = rng.uniform(-math.pi, math.pi)
        X[i, :2] = wps[idx[i], :2] + rng.uniform(0.05, 0.25) * np.array([math.cos(ang), math.sin(ang)])
    goal = c["goal"].copy()
    has = goal[:, 3] != 0
    goal[has, :npos] = wps[idx[has], :npos]
    n_wp = c["n_wp"].copy()
    n_wp[0] = 3
    assert (n_wp[1:] != 3).any()
    c.update(X=X, wp_index=idx, goal=goal, waypoints=wps, n_wp=n_wp, n_wp_shared=3)
    return c


def f32_rounded(c):
    """The batch as f32 storage holds it, as doubles."""
    c = dict(c)
    for k in ("X", "goal", "waypoints", "u", "u_last", "table"):
        c[k] = c[k].astype(np.float32).astype(np.float64)
    return c


def run_oracle(c, cfg, idx=None, table=None, apply=True):
    """select() and apply(u) of oracle/tracking_quad.py on every agent of `c` (or on those of `idx`) under launch configuration `cfg`.
    Frozen agents (ret_in != 0) are not run: a launch leaves them as they are.  Returns what the kernels write, [n, ...] arrays:
    sm, wp_index, goal [n,4] (a goal that becomes invalid keeps its stored coordinates), obs_out [n,K,7], goal_out, u_ref, track, ret,
    ret_step, X, u_last; stepped / hit_before / hit_after; margins: threshold name -> [n] (inf where no such comparison was made);
    order_ties [n]: exact distance ties among the rows kept."""
    model = c["model"]
    nx, nu, npos = dims(model)
    table = c["table"][: cfg["M"]] if table is None else table
    idx = np.arange(len(c["X"])) if idx is None else np.asarray(idx)
    n, K = len(idx), cfg["K"]
    o = T.QuadTrackingOracle(model, np.zeros(nx), dict(reached_threshold=cfg["reached_threshold"]), dt=DT, obs=table, num_constraints=K,
                             enable_rotation=bool(cfg["enable_rotation"]))
    shared = c["waypoints"].ndim == 2
    r = dict(sm=c["sm"][idx].copy(), wp_index=c["wp_index"][idx].copy(), goal=c["goal"][idx].copy(), obs_out=np.zeros((n, K, 7)),
             goal_out=np.zeros((n, npos)), u_ref=np.zeros((n, nu)), track=np.zeros(n, dtype=np.int32), ret=c["ret_in"][idx].copy(),
             ret_step=c["ret_step_in"][idx].copy(), X=c["X"][idx].copy(), u_last=c["u_last"][idx].copy(),
             stepped=np.zeros(n, dtype=bool), hit_before=np.zeros(n, dtype=bool), hit_after=np.zeros(n, dtype=bool),
             order_ties=np.zeros(n, dtype=int), running=c["ret_in"][idx] == 0, margins={})
    for j, i in enumerate(idx):
        if c["ret_in"][i] != 0:
            continue
        nw = c["n_wp_shared"] if shared else int(c["n_wp"][i])
        o.X = c["X"][i].copy()
        o.state_machine = SM_NAMES[c["sm"][i]]
        o.goal = c["goal"][i, :npos].copy() if c["goal"][i, 3] != 0 else None
        o.current_goal_index = int(c["wp_index"][i])
        o.waypoints = (c["waypoints"] if shared else c["waypoints"][i])[:nw, :npos]
        o.u_pos, o.margins = None, {}
        s = o.select()
        r["sm"][j], r["wp_index"][j], r["track"][j] = SM_NAMES.index(s["state_machine"]), s["index"], int(s["track"])
        if s["goal"] is None:
            r["goal"][j, 3] = 0.0
        else:
            r["goal"][j, :npos], r["goal"][j, 3] = s["goal"], 1.0
        r["obs_out"][j], r["goal_out"][j], r["u_ref"][j] = s["obs"], s["goal_out"], s["u_ref"]
        if apply:
            ret = o.apply(c["u"][i].copy())
            r["stepped"][j] = o.u_pos is not None
            r["hit_before"][j], r["hit_after"][j] = ret == -2 and not r["stepped"][j], ret == -2 and r["stepped"][j]
            r["ret"][j], r["X"][j] = ret, o.X
            if r["stepped"][j]:
                r["u_last"][j] = o.u_pos
            if ret != 0:
                r["ret_step"][j] = STEP_INDEX
        r["order_ties"][j] = o.margins.pop("order_ties", 0)
        for name, v in o.margins.items():
            r["margins"].setdefault(name, np.full(n, np.inf))[j] = v
    return r


@functools.lru_cache(maxsize=None)
def reference(model, cfg_index, kind="main", f32=False, n=None):
    """run_oracle, computed once per process: configuration CONFIGS[cfg_index] (or BIG for cfg_index == -1: the first n agents over
    big_table(), select only), the per-agent batch ('main') or the shared-waypoint one ('shared'), the inputs as given or f32-rounded."""
    c = cases(model) if kind == "main" else shared_cases(model)
    if cfg_index == -1:
        c = dict(c, table=big_table())
    if f32:
        c = f32_rounded(c)
    if cfg_index == -1:
        return run_oracle(c, BIG, idx=np.arange(n), table=c["table"], apply=False)
    return run_oracle(c, CONFIGS[cfg_index], idx=None if n is None else np.arange(n))


N_SUB = 65                                       # the sub-selection: the first 65 agents of the shuffled batch (one wave and a lane)
# every oracle run the GPU tests compare a launch with, as arguments of reference(): the four full-table configurations on the whole
# batch, two of them in f32 storage as well; the K x M edges on the sub-selection; the shared waypoint list; the largest table
USED = tuple((i, "main", False, None) for i in range(len(MAIN))) + ((0, "main", True, None), (1, "main", True, None)) \
    + tuple((len(MAIN) + i, "main", False, N_SUB) for i in range(len(EDGE))) + ((0, "shared", False, None), (-1, "main", False, N_SUB))


def exact_allowed(c):
    """threshold name -> agents allowed to sit exactly on it."""
    z = np.zeros(len(c["X"]), dtype=bool)
    return {"reached": c["placed"]["exact_reached"], "order": z}


def margin_violations(c, r, idx=None):
    """[(threshold, agent, margin)] for every comparison closer than MARGIN to its threshold that is not an allowed exact case (margin
    exactly 0 on an agent built for it)."""
    idx = np.arange(len(c["X"])) if idx is None else idx
    bad = []
    for name, m in r["margins"].items():
        ok0 = exact_allowed(c).get(name, np.zeros(len(c["X"]), dtype=bool))[idx]
        for j in np.flatnonzero((m <= MARGIN) & ~((m == 0.0) & ok0)):
            bad.append((name, int(idx[j]), float(m[j])))
    return bad


def tags(model):
    """name -> agent mask over the main batch: what the oracle did with each agent under MAIN[0] (enable_rotation 1) and MAIN[1]
    (enable_rotation 0).  Every one of them has to be populated (tests/test_quadtrack_cases.py)."""
    c = cases(model)
    q3, vt = model == "Quad3D", model == "VTOL2D"
    t = {}
    run = c["ret_in"] == 0
    for e, ci in ((1, 0), (0, 1)):
        r = reference(model, ci)
        sm0, sm1 = c["sm"], r["sm"]
        for s, name in enumerate(SM_NAMES):
            t[f"enters_{name}"] = run & (sm0 == s)
        vel = c["X"][:, 6:9] if q3 else c["X"][:, 3:5]
        lin = np.linalg.norm(vel, axis=1) < 0.05
        ang = np.linalg.norm(c["X"][:, 9:12], axis=1) < 0.05 if q3 else np.ones(len(lin), dtype=bool)
        stop = run & (sm0 == STOP)
        t[f"rot{e}_stop_has_stopped"] = stop & (sm1 != STOP)
        t[f"rot{e}_stop_still_moving"] = stop & (sm1 == STOP)
        assert np.array_equal(stop & lin & ang, t[f"rot{e}_stop_has_stopped"])
        if q3:
            t["stop_linear_slow_angular_fast"], t["stop_linear_fast_angular_slow"] = stop & lin & ~ang, stop & ~lin & ang
            t["stop_both_fast"] = stop & ~lin & ~ang
        # 'rotate' (entered in it, or reached from 'stop'): the heading against the bearing of the waypoint
        turned = run & np.isfinite(r["margins"].get("rotation", np.full(len(run), np.inf)))
        yaw = c["X"][:, 5] if q3 else c["X"][:, 2]
        w = c["waypoints"][np.arange(len(run)), np.minimum(c["wp_index"], c["n_wp"] - 1)]
        inside = np.abs(yaw - np.arctan2(w[:, 1] - c["X"][:, 1], w[:, 0] - c["X"][:, 0])) <= 0.1
        t[f"rot{e}_rotate_inside_threshold"], t[f"rot{e}_rotate_outside_threshold"] = turned & inside, turned & ~inside
        if q3 and e:
            t["stays_in_rotate"] = turned & (sm1 == ROTATE)
        t[f"rot{e}_waypoint_advanced"] = run & (r["wp_index"] == c["wp_index"] + 1) & (sm1 != IDLE)
        t[f"rot{e}_last_waypoint_to_idle"] = run & (sm0 != IDLE) & (sm1 == IDLE)
        t[f"rot{e}_goal_valid_ret_0"] = run & (r["goal"][:, 3] != 0) & (r["ret"] == 0)
        t[f"rot{e}_no_goal_ret_minus_1"] = run & (r["goal"][:, 3] == 0) & (r["ret"] == -1)
        t[f"rot{e}_no_goal_in_stop_ret_0"] = run & (r["goal"][:, 3] == 0) & (sm1 == STOP) & (r["ret"] == 0)
        t[f"rot{e}_track_flag"] = run & (r["track"] == 1)
    r = reference(model, 0)
    P = c["placed"]
    t["hit_before_circle"] = r["hit_before"] & (P["in_circle"] | P["in_flag1_circle"])
    t["hit_before_flag1_low_exponent"] = r["hit_before"] & P["in_flag1_circle"]
    t["hit_before_superell"] = r["hit_before"] & P["in_superell"]
    for e in (2.0, 4.0, 2.5):
        rows = [m for m in range(M_TABLE) if is_superell(c["table"][m]) and c["table"][m, 4] == e]
        near = np.array([min(np.linalg.norm(x[:2] - c["table"][m, :2]) for m in rows) < 1.2 for x in c["X"]])
        t[f"hit_before_superell_exponent_{e}"] = t["hit_before_superell"] & near
    t["superell_nan_no_hit"] = run & P["in_superell_nan"] & ~r["hit_before"]
    t["hit_after_circle"] = r["hit_after"] & P["towards_circle"]
    t["hit_after_superell"] = r["hit_after"] & P["towards_superell"]
    t["no_hit"] = run & r["stepped"] & ~r["hit_after"]
    t["frozen_minus_1"], t["frozen_minus_2"] = c["ret_in"] == -1, c["ret_in"] == -2
    t["exact_tie"], t["exact_reached"] = run & P["exact_tie"] & (r["order_ties"] >= 2), run & P["exact_reached"]
    t["tie_shared_centre"] = run & ~P["exact_tie"] & (r["order_ties"] >= 1)
    lo, hi = u_box(model)
    t["input_outside_box"] = run & ((c["u"] < lo) | (c["u"] > hi)).any(axis=1)
    t["input_inside_box"] = run & ~t["input_outside_box"]
    for k in ((3, 4, 5) if q3 else (2,)):
        at = r["stepped"] & (np.abs(c["X"][:, k]) > math.pi - 2e-3) & (np.abs(c["X"][:, k]) < math.pi)
        t[f"angle_{k}_wraps"] = at & (np.sign(r["X"][:, k]) != np.sign(c["X"][:, k]))
        t[f"angle_{k}_near_pi_no_wrap"] = at & (np.sign(r["X"][:, k]) == np.sign(c["X"][:, k]))
    for name in ("n_wp_1", "n_wp_2", "n_wp_3", "n_wp_4"):
        t[name] = run & (c["n_wp"] == int(name[-1]))
    if not vt:
        clipped = run & ((r["u_ref"] == lo) | (r["u_ref"] == hi)).any(axis=1)
        t["u_ref_clipped"], t["u_ref_unclipped"] = clipped, run & ~clipped
    if vt:
        K = CONFIGS[0]["K"]
        tb = c["table"]
        off = np.abs(T.R.angle_normalize(np.arctan2(tb[None, :, 1] - c["X"][:, 1:2], tb[None, :, 0] - c["X"][:, 0:1]) - c["X"][:, 2:3]))
        inside = (off <= 0.6 * np.pi).sum(axis=1)
        t["cone_empty_fallback"], t["cone_fewer_than_K"] = run & (inside == 0), run & (inside > 0) & (inside < K)
        t["cone_K_or_more"], t["cone_some_left_out"] = run & (inside >= K), run & (inside > 0) & (inside < M_TABLE)
        t["below_ground_before"] = r["hit_before"] & (c["X"][:, 1] < 0)
        t["below_ground_after"] = r["hit_after"] & (r["X"][:, 1] < 0) & P["towards_ground"]
        t["past_pitch_limit"] = r["hit_before"] & (np.abs(c["X"][:, 2]) > 15.0)
    return t
