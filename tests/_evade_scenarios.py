"""Scenarios of the evade example for the Backup-CBF and shield tests.  TEST INFRASTRUCTURE ONLY.

"default" is the scenario examples/evade/test_evade.py ships; many of its parameters coincide (radius == safety_margin,
a_max == Kp == Kd == alpha_terminal == 2, alpha == 1, hallway == pocket == bullet width, bullet speed == length == 3), so
a kernel or a host layer that reads the wrong field passes every test run on it.  Scenario "B" keeps every such pair
apart and away from the literals of the reference's evade code (0.1, 0.2, 1.0, 2.0, 3.0); the reference can build it
(EvadeEnv's constructor arguments, the robot spec, the two gains of EvadeBackupController and the two decay rates of
BackupCBF), so tests/golden/backup_cbf_b.npz and shield_b.npz pin it on the reference's own run.

The golden scripts and the tests import the numbers, the draws and the wrong-field "confusions" from here, and
``solve_many`` / ``loops_many`` run oracle.backup_cbf over a batch in plain child processes
(``python tests/_evade_scenarios.py in.npz out.npz``), never a fork of a process that may hold a HIP context.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import backup_cbf as O  # noqa: E402
from oracle import qp as oqp  # noqa: E402

# ---- the numbers ------------------------------------------------------------------------------------------------------------
ENV_KW = {
    "default": dict(hallway_length=60.0, hallway_width=4.0, pocket_x=25.0, pocket_length=10.0, pocket_width=4.0, goal_length=5.0,
                    bullet_speed=3.0, bullet_length=3.0, bullet_width=None, bullet_start_x=-10.0),
    "B": dict(hallway_length=72.0, hallway_width=5.0, pocket_x=31.0, pocket_length=12.0, pocket_width=3.5, goal_length=6.0,
              bullet_speed=2.6, bullet_length=3.6, bullet_width=4.2, bullet_start_x=-7.0),
}
ROBOT = {"default": dict(radius=0.5, a_max=2.0, v_max=1.5, safety_margin=0.5),
         "B": dict(radius=0.4, a_max=2.4, v_max=1.7, safety_margin=0.3)}
CBF = {"default": dict(alpha=1.0, alpha_terminal=2.0), "B": dict(alpha=0.8, alpha_terminal=1.6)}
GAINS = {"default": dict(kp=2.0, kd=2.0), "B": dict(kp=1.5, kd=2.5)}
DT = {"default": 0.1, "B": 0.1}
HORIZON = {"default": 12.0, "B": 9.0}                       # backup horizon: N = 120 and N = 90

ENV_VECTOR = ("hallway_length", "half_width", "pocket_x_min", "pocket_x_max", "pocket_y_min", "pocket_y_max", "goal_x_min",
              "goal_x_max", "bullet_speed", "bullet_length", "bullet_width", "bullet_start_x")


def oracle_env(name="B", **over):
    """The oracle's environment dict of a scenario (oracle.backup_cbf.default_env)."""
    return O.default_env(**{**ENV_KW[name], **over})


def oracle_spec(name="B", **over):
    """The oracle's spec: robot, decay rates and the backup controller's gains."""
    return O.default_spec(**{**ROBOT[name], **CBF[name], **GAINS[name], **over})


def kernel_env(name="B"):
    """The environment dict BatchedBackupCBF / BatchedShield take."""
    from safe_control_amd.position_control.backup_cbf_qp import default_evade_env
    return default_evade_env(**ENV_KW[name])


BATCH, BATCH_SEED = 192, 1                                   # the drawn batch of the GPU tests and of the confusion test
FAR = 1.0e12                                                 # ulp(FAR) = 1.2e-4 > the forward-difference step 1e-5


# ---- draws at scenario B ----------------------------------------------------------------------------------------------------
def draw_call_b(rng, kind):
    """The five kinds of make_golden_backup.py / make_golden_shield.py, their x-ranges moved to B's pocket (31..43, y 2.5..6)
    and goal zone (66..72)."""
    if kind == 0:      # hallway, bullet close behind
        x = np.array([rng.uniform(8, 60), rng.uniform(-1.7, 1.7), rng.uniform(0, 1.7), rng.uniform(-0.3, 0.3)])
        bx = x[0] - rng.uniform(4, 14)
    elif kind == 1:    # below the pocket
        x = np.array([rng.uniform(32.5, 41.5), rng.uniform(-1.5, 1.9), rng.uniform(-0.5, 1.0), rng.uniform(-0.3, 0.8)])
        bx = x[0] - rng.uniform(3, 20)
    elif kind == 2:    # inside the pocket
        x = np.array([rng.uniform(32.5, 41.5), rng.uniform(3.2, 5.4), rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4)])
        bx = rng.uniform(0, 72)
    elif kind == 3:    # bullet far away or ahead
        x = np.array([rng.uniform(5, 60), rng.uniform(-1.5, 1.5), rng.uniform(0.5, 1.7), rng.uniform(-0.2, 0.2)])
        bx = x[0] + rng.uniform(6, 20) if rng.uniform() < 0.5 else ENV_KW["B"]["bullet_start_x"]
    else:              # around the left edge of the goal zone
        x = np.array([rng.uniform(61, 70.5), rng.uniform(-1.5, 1.5), rng.uniform(0.0, 1.7), rng.uniform(-0.2, 0.2)])
        bx = x[0] - rng.uniform(5, 30)
    return x, bx


def draw_calls_b(B, seed):
    """B single-call situations, kind i % 5."""
    rng = np.random.default_rng(seed)
    xs, bs = zip(*(draw_call_b(rng, i % 5) for i in range(B)))
    return np.array(xs), np.array(bs)


def draw_states_b(B, seed):
    """test_backupcbf_gpu.draw_states scaled to scenario B: the hallway, ~30 % over / in the pocket, and a fifth of the agents
    within 1.5 m of the goal zone's left edge (x = 66; the backup controller brakes inside the zone and steers back to the
    pocket outside it).  Also a user reference input per agent, a quarter of them outside the +-a_max box."""
    rng = np.random.default_rng(seed)
    X = np.column_stack([rng.uniform(2, 70, B), rng.uniform(-1.9, 1.9, B), rng.uniform(-0.5, 1.7, B), rng.uniform(-0.5, 0.5, B)])
    r = rng.uniform(size=B)
    pocket = r < 0.3
    X[pocket, 0] = rng.uniform(31.6, 42.4, pocket.sum())
    X[pocket, 1] = rng.uniform(-1.5, 5.5, pocket.sum())
    goal = r > 0.8
    X[goal, 0] = rng.uniform(65.0, 67.2, goal.sum())
    bx = X[:, 0] - rng.uniform(-10, 25, B)
    a = ROBOT["B"]["a_max"]
    u_nom = rng.uniform(-a, a, (B, 2))
    wide = rng.uniform(size=B) < 0.25
    u_nom[wide] *= rng.uniform(1.1, 2.0, (int(wide.sum()), 1))
    # No row survives the keep rule only where every forward difference of h vanishes.  Inside the map that cannot last a whole
    # horizon (the first rows have |lhs| = dt |grad h| and grad h is a unit vector outside the bullet's box), so the no-rows
    # branch -- status -1, the reference input returned UNCLIPPED -- is reached by agents so far outside that x + 1e-5 == x.
    if B >= 16:
        X[-4:, :2] = [[FAR, 0.3], [-FAR, -0.2], [40.0, FAR], [12.0, -FAR]]
        u_nom[-4:] = [[3.1, -0.4], [-2.9, 5.0], [0.2, 2.6], [-7.0, -7.0]]
    return X, bx, u_nom


def draw_loop_starts_b(B, seed):
    """Starts of short closed loops: a third within a braking distance of the goal zone with the bullet far behind (they arrive;
    from farther away the infeasible QP hands over to the backup controller, which turns back to the pocket), a third
    with the bullet's nose a few metres behind them in the open hallway (it catches them), the rest anywhere with the bullet
    late in its pass (it leaves the hallway and respawns)."""
    rng = np.random.default_rng(seed)
    X = np.zeros((B, 4))
    bx = np.zeros(B)
    for i in range(B):
        k = i % 3
        if k == 0:
            X[i] = [rng.uniform(65.55, 66.3), rng.uniform(-1.0, 1.0), rng.uniform(1.5, 1.7), rng.uniform(-0.1, 0.1)]
            bx[i] = rng.uniform(-7, 10)
        elif k == 1:
            X[i] = [rng.uniform(8, 24), rng.uniform(-1.5, 1.5), rng.uniform(0.0, 1.5), rng.uniform(-0.2, 0.2)]
            bx[i] = X[i, 0] - rng.uniform(3.5, 7.0)
        else:
            X[i] = [rng.uniform(5, 60), rng.uniform(-1.5, 1.5), rng.uniform(0.0, 1.5), rng.uniform(-0.2, 0.2)]
            bx[i] = rng.uniform(70, 75.4)
    return X, bx


# ---- wrong-field confusions -------------------------------------------------------------------------------------------------
def confusions():
    """name -> (env, spec) of scenario B as a kernel or host layer that reads the wrong field would see it."""
    kw, rb, cb, gn = ENV_KW["B"], ROBOT["B"], CBF["B"], GAINS["B"]
    return {
        "bullet_width := hallway_width": (oracle_env(bullet_width=kw["hallway_width"]), oracle_spec()),
        "kp <-> kd": (oracle_env(), oracle_spec(kp=gn["kd"], kd=gn["kp"])),
        "radius <-> safety_margin": (oracle_env(), oracle_spec(radius=rb["safety_margin"], safety_margin=rb["radius"])),
        "alpha := 1": (oracle_env(), oracle_spec(alpha=1.0)),
        "pocket_width := hallway_width": (oracle_env(pocket_width=kw["hallway_width"]), oracle_spec()),
        "bullet_speed := bullet_length": (oracle_env(bullet_speed=kw["bullet_length"]), oracle_spec()),
        "alpha_terminal := a_max": (oracle_env(), oracle_spec(alpha_terminal=rb["a_max"])),
        "goal_length := 5": (oracle_env(goal_length=5.0), oracle_spec()),
        "kd := a_max": (oracle_env(), oracle_spec(kd=rb["a_max"])),
    }


# ---- the oracle over a batch ------------------------------------------------------------------------------------------------
KEEP = 1e-6                                                  # the reference's keep rule |lhs| > 1e-6 (backup_cbf_qp.py:663-665)


def solve_one(x, u_nom, bx, dt, horizon, env, spec):
    """oracle.backup_cbf.solve plus what the set-aside rule needs: the feasibility margin of the stated QP (NaN without one)
    and the smallest distance of a row's |lhs| from the keep threshold."""
    seen = {}
    inner = O.assemble_rows

    def recording(*a):
        r = inner(*a)
        seen["lhs"] = r[0]
        return r

    O.assemble_rows = recording
    try:
        if u_nom is None or np.isnan(u_nom).any():
            u_nom = O.nominal_control(x, spec)
        u, info = O.solve(x, u_nom, bx, dt, horizon, env, spec, return_info=True)
    finally:
        O.assemble_rows = inner
    rows, n = info["rows"], info["n_rows"]
    margin = np.nan
    if n > 0 and np.all(np.isfinite(rows)):
        A = np.vstack([rows[:, :2], np.eye(2), -np.eye(2)])
        margin = oqp.feasibility_margin(A, np.concatenate([-rows[:, 2], np.ones(4)]))
    nrm = np.sqrt((seen["lhs"] ** 2).sum(axis=1))
    gap = np.abs(nrm - KEEP)
    return dict(u=u, status=info["qp_status"], using_backup=info["using_backup"], h_min=info["h_min"], n_rows=n, rows=rows,
                margin=margin, keep_gap=float(np.nanmin(gap)) if np.isfinite(gap).any() else np.nan)


def loop_one(x0, bx0, steps, dt, horizon, env, spec):
    """oracle.backup_cbf.closed_loop plus the feasibility margin of every step's QP."""
    margins, status = [], []
    inner = O.solve

    def recording(*a, **kw):
        u, info = inner(*a, **kw)
        rows = info["rows"]
        m = np.nan
        if info["n_rows"] > 0 and np.all(np.isfinite(rows)):
            m = oqp.feasibility_margin(np.vstack([rows[:, :2], np.eye(2), -np.eye(2)]), np.concatenate([-rows[:, 2], np.ones(4)]))
        margins.append(m)
        status.append(info["qp_status"])
        return u, info

    O.solve = recording
    try:
        Xs, Us, Bs, UB, HM, outcome, xf = O.closed_loop(x0, bx0, steps, dt, horizon, env, spec)
    finally:
        O.solve = inner
    T = len(Xs)
    pad = lambda a, w: np.concatenate([np.asarray(a, dtype=float).reshape(T, *w), np.full((steps - T, *w), np.nan)])
    return dict(X=pad(Xs, (4,)), U=pad(Us, (2,)), bullet=pad(Bs, ()), margin=pad(margins, ()), status=pad(status, ()), n=T, ret=outcome,
                ret_step=T - 1 if outcome != 0 else -1, x_final=xf)


# ---- the comparison of the GPU tests (and what the confusion test calls a change) -------------------------------------------
ROW_TOL, U_TOL, H_TOL = 1e-7, 1e-6, 1e-9                     # tests/test_backupcbf_gpu.py, float64 storage


def compare(got, ref, stored_eps=0.0):
    """Per agent: (flip, differs).  flip: n_rows or status disagree (what the set-aside rule may excuse).  differs: anything the
    GPU test compares disagrees -- kept rows beyond ROW_TOL max(1, |row|_inf), u beyond U_TOL, h_min beyond H_TOL, n_rows,
    status, using_backup.  stored_eps (2^-23 for float32 storage) adds one rounding of the stored u and h_min."""
    B = len(ref["u"])
    flip = (got["n_rows"] != ref["n_rows"]) | (got["status"] != ref["status"])
    differs = flip | (got["using_backup"].astype(bool) != ref["using_backup"].astype(bool))
    differs |= ~(np.abs(got["h_min"] - ref["h_min"]) <= H_TOL + stored_eps * np.maximum(1.0, np.abs(ref["h_min"])))
    differs |= ~np.all(np.abs(got["u"] - ref["u"]) <= U_TOL + stored_eps * np.maximum(1.0, np.abs(ref["u"])), axis=1)
    for i in range(B):
        n = int(ref["n_rows"][i])
        if n > 0 and not flip[i]:
            r = ref["rows"][i][:n]
            differs[i] |= not (np.abs(got["rows"][i][:n] - r).max() <= ROW_TOL * max(1.0, np.abs(r).max()))
    return flip, differs


def may_set_aside(ref):
    """Per agent: the oracle's QP is within 1e-6 of flipping between feasible and infeasible, or a row's |lhs| is within 1e-9
    of the keep threshold."""
    return (np.abs(ref["margin"]) < 1e-6) | (ref["keep_gap"] <= 1e-9)


MAX_WORKERS = 16


def _worker(inp, outp):
    d = np.load(inp)
    env, spec = json.loads(str(d["env"])), json.loads(str(d["spec"]))
    dt, horizon = float(d["dt"]), float(d["horizon"])
    if str(d["kind"]) == "solve":
        res = [solve_one(x, un, bx, dt, horizon, env, spec) for x, un, bx in zip(d["X"], d["u_nom"], d["bx"])]
        N = int(horizon / dt)
        for r in res:
            rows = np.zeros((N, 3))
            rows[: r["n_rows"]] = r["rows"]
            r["rows"] = rows
    else:
        res = [loop_one(x, bx, int(d["steps"]), dt, horizon, env, spec) for x, bx in zip(d["X"], d["bx"])]
    np.savez(outp, **{k: np.array([r[k] for r in res]) for k in res[0]})


def _run(kind, X, bx, dt, horizon, env, spec, workers, timeout, **extra):
    n = max(1, min(int(workers or MAX_WORKERS), MAX_WORKERS, os.cpu_count() or 2, len(X)))
    parts = np.array_split(np.arange(len(X)), n)
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for j, idx in enumerate(parts):
            inp, outp = os.path.join(tmp, f"in{j}.npz"), os.path.join(tmp, f"out{j}.npz")
            np.savez(inp, kind=kind, X=X[idx], bx=bx[idx], dt=dt, horizon=horizon, env=json.dumps(env), spec=json.dumps(spec),
                     **{k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in extra.items()})
            penv = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
            procs.append((subprocess.Popen([sys.executable, os.path.abspath(__file__), inp, outp], env=penv), outp))
        for p, _ in procs:
            if p.wait(timeout=timeout) != 0:
                raise RuntimeError("Backup-CBF oracle worker failed")
        res = [np.load(o) for _, o in procs]
        return {k: np.concatenate([r[k] for r in res]) for k in res[0].files}


def solve_many(X, u_nom, bx, dt, horizon, env, spec, workers=None, timeout=900):
    """solve_one for every row (u_nom None or a NaN row: the example's nominal controller); dict of arrays, rows padded to
    [B, N, 3] with zeros."""
    X, bx = np.asarray(X, dtype=float), np.asarray(bx, dtype=float)
    un = np.full((len(X), 2), np.nan) if u_nom is None else np.asarray(u_nom, dtype=float)
    return _run("solve", X, bx, dt, horizon, env, spec, workers, timeout, u_nom=un)


def loops_many(X0, bx0, steps, dt, horizon, env, spec, workers=None, timeout=900):
    """loop_one for every row; dict of arrays, the per-step ones padded with NaN to `steps`."""
    return _run("loop", np.asarray(X0, dtype=float), np.asarray(bx0, dtype=float), dt, horizon, env, spec, workers, timeout,
                steps=int(steps))


if __name__ == "__main__":
    _worker(sys.argv[1], sys.argv[2])
