#!/usr/bin/env python3
"""What per-agent parameters cost: the `_agents` entry points beside their scalar siblings, in one job, launches alternated.

Fused loop (sc_tracking_rollout_batch / sc_tracking_rollout_batch_agents): the 14-circle scene of tests/golden/closed_loop.npz,
B = 4096 and 65536 DynamicUnicycle2D agents x 200 control steps in ONE launch, under the default (cooperative) dispatch and under
SC_TRACK_LANE_PER_AGENT=1:
  scalar    one robot_spec for the batch: the yardstick (the parent commit's path, unchanged)
  uniform   the per-agent kernel, every agent's row equal to the struct: same arithmetic, ten more 8-byte loads per agent
  drawn     the per-agent kernel, alpha1 / alpha2 in 0.5 .. 3, a_max in 0.5 .. 1.5, radius in 0.2 .. 0.35 per agent (other runs:
            agents end at other steps, so this row is not comparable step for step)
Solve (sc_cbfqp_solve_batch with SC_CBFQP_GENERIC=1 / sc_cbfqp_solve_batch_agents): B = 4096 and 2^20 agents x 8 obstacles.  The
scalar call picks its kernel by batch size (cooperative up to 32768 agents, the register kernel above); the per-agent call is one
QP per lane at every size.

HIP events around each launch, one warm-up round, then `reps` rounds in which the variants take turns (scalar, uniform, drawn,
scalar, ..), median (min .. max) per variant; the ratio is median over median and the yardstick's own range is printed beside it.

Usage: python tools/time_agent_params.py [steps] [reps]"""
import os
import statistics
import sys

os.environ.setdefault("SC_CBFQP_GENERIC", "1")                    # read once by the library: set before it loads

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import safe_control_amd as sca  # noqa: E402
from safe_control_amd import workloads as W  # noqa: E402

SPEC = {"model": "DynamicUnicycle2D", "a_max": 1.0, "w_max": 0.5, "radius": 0.25, "cbf_alpha1": 1.5, "cbf_alpha2": 1.5}
STATE = ("X", "state_machine", "current_goal_index", "goal", "ret", "ret_step", "u_pos")
DEV = "cuda:0"


def scene():
    g = np.load(os.path.join(ROOT, "tests", "golden", "closed_loop.npz"))
    return g["du14/obs"], g["du14/waypoints"][:, :2]


def starts(B, seed=1):
    rng = np.random.default_rng(seed)
    return np.column_stack([2.0 + rng.uniform(-0.4, 0.4, (B, 2)), rng.uniform(-np.pi, np.pi, B), rng.uniform(0.1, 1.0, B)])


def agent_specs(B, drawn, seed=2):
    """robot_spec and agent_spec of the `uniform` (every row = SPEC) and `drawn` variants.  A grid of 4096 distinct agents, tiled:
    what a sweep looks like, and the host builds its table in one pass per distinct agent."""
    shared = {k: v for k, v in SPEC.items() if k not in ("a_max", "radius", "cbf_alpha1", "cbf_alpha2")}
    rng = np.random.default_rng(seed)
    n = min(B, 4096)
    cols = {"cbf_alpha1": rng.uniform(0.5, 3.0, n), "cbf_alpha2": rng.uniform(0.5, 3.0, n), "a_max": rng.uniform(0.5, 1.5, n),
            "radius": rng.uniform(0.2, 0.35, n)}
    if not drawn:
        cols = {k: np.full(n, SPEC[k]) for k in cols}
    return shared, {k: np.tile(v, B // n) for k, v in cols.items()}


def summary(ms):
    return statistics.median(ms), min(ms), max(ms)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def report(tag, B, times, unit):
    y = summary(times["scalar"])
    print(f"{tag} B={B:8d} scalar   {y[0]:9.4f} {unit} ({y[1]:.4f} .. {y[2]:.4f})  range {100 * (y[2] - y[1]) / y[0]:.1f} % of the median")
    for name in ("uniform", "drawn"):
        if name in times:
            t = summary(times[name])
            print(f"{tag} B={B:8d} {name:8s} {t[0]:9.4f} {unit} ({t[1]:.4f} .. {t[2]:.4f})  x{t[0] / y[0]:.4f} of scalar", flush=True)


def time_rollouts(B, steps, reps, obs, wps):
    X0 = starts(B)
    ctls = {"scalar": sca.BatchedTrackingController(X0, dict(SPEC), obs=obs)}
    for name, drawn in (("uniform", False), ("drawn", True)):
        shared, agent = agent_specs(B, drawn)
        ctls[name] = sca.BatchedTrackingController(X0, shared, obs=obs, agent_spec=agent)
    saved = {}
    for name, c in ctls.items():
        c.set_waypoints(wps)                                       # prepared on the host, once
        saved[name] = {n: getattr(c, n).clone() for n in STATE}
    times = {name: [] for name in ctls}
    for rep in range(reps + 1):
        for name, c in ctls.items():                               # the variants take turns within a round
            for n in STATE:
                getattr(c, n).copy_(saved[name][n])
            c.steps_done = 0
            ms = timed(lambda: c.control_step(steps))
            if rep > 0:                                            # round 0 is the warm-up
                times[name].append(ms)
    ended = {name: int((c.ret != 0).sum()) for name, c in ctls.items()}
    same = all(torch.equal(getattr(ctls["scalar"], n), getattr(ctls["uniform"], n)) for n in ("X", "ret", "ret_step"))
    return times, ended, same


def time_solves(B, reps):
    X, goal, u_ref, obs = W.du_cbfqp_batch(B, 8, seed=3)
    t64 = lambda a: torch.tensor(a, dtype=torch.float64, device=DEV)
    tX, tu, to = t64(X), t64(u_ref), t64(obs)
    ctls = {"scalar": sca.BatchedCBFQP(dict(SPEC), io_dtype="f64", compute_dtype="f64")}
    for name, drawn in (("uniform", False), ("drawn", True)):
        shared, agent = agent_specs(B, drawn)
        ctls[name] = sca.BatchedCBFQP(shared, io_dtype="f64", compute_dtype="f64", agent_spec=agent)
    outs = {name: c.solve(tX, tu, to) for name, c in ctls.items()}          # allocates the outputs and uploads the tables
    times = {name: [] for name in ctls}
    for rep in range(reps + 1):
        for name, c in ctls.items():
            ms = timed(lambda: c.solve(tX, tu, to, out=outs[name]))
            if rep > 0:
                times[name].append(1e3 * ms)
    torch.cuda.synchronize()
    us, ss, _ = outs["scalar"]
    uu, su, _ = outs["uniform"]
    ok = ss == 0
    worst = float((uu[ok] - us[ok]).abs().max()) if bool(torch.equal(ss, su)) else float("nan")
    return times, worst


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    obs, wps = scene()
    for mode, tag in ((None, "rollout coop "), ("1", "rollout lane ")):
        if mode:
            os.environ["SC_TRACK_LANE_PER_AGENT"] = mode
        try:
            for B in (4096, 65536):
                times, ended, same = time_rollouts(B, steps, reps, obs, wps)
                report(tag, B, times, f"ms/{steps} steps")
                print(f"{tag} B={B:8d} agents ended: {ended}; uniform == scalar bit for bit: {same}", flush=True)
        finally:
            os.environ.pop("SC_TRACK_LANE_PER_AGENT", None)
    for B in (4096, 1 << 20):
        times, worst = time_solves(B, reps)
        report("solve K=8     ", B, times, "us")
        print(f"solve K=8      B={B:8d} max |u_uniform - u_scalar| over optimal agents: {worst:.2e}", flush=True)


if __name__ == "__main__":
    main()
