#!/usr/bin/env python3
"""ms per launch of the optimal-decay closed loop (sc_tracking_od_rollout_batch, csrc/tracking_od.hip) beside the lane-per-agent
'cbf_qp' rollout with ONE constraint row (sc_tracking_rollout_batch with num_constraints = 1 and SC_TRACK_LANE_PER_AGENT=1), on the
14-circle scene of tests/golden/closed_loop.npz: B = 4096 and 65536 agents x 200 control steps in one launch, HIP events around the
launch, one warm-up launch, median (and min .. max) of the repeated runs.

  cbf_qp/1   the existing lane-per-agent rollout, one row: the yardstick             (1)
  od         the optimal-decay rollout: same state machine, table scan, collision    (2)
             tests and step; a running minimum instead of the sorted insertion, the
             1 + 9 active-set solve with two decay variables instead of the 2-D walk

Usage: python tools/time_od_loop.py [steps] [reps]"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import safe_control_amd as sca  # noqa: E402

SPECS = {"DynamicUnicycle2D": {"model": "DynamicUnicycle2D", "a_max": 1.0, "w_max": 0.5, "radius": 0.25},
         "KinematicBicycle2D_C3BF": {"model": "KinematicBicycle2D_C3BF", "a_max": 5.0, "radius": 0.3}}
STATE = ("X", "state_machine", "current_goal_index", "goal", "ret", "ret_step", "u_pos", "omega", "min_h")


def scene():
    g = np.load(os.path.join(ROOT, "tests", "golden", "closed_loop.npz"))
    return g["du14/obs"], g["du14/waypoints"][:, :2]


def starts(B, seed=1):
    rng = np.random.default_rng(seed)
    return np.column_stack([2.0 + rng.uniform(-0.4, 0.4, (B, 2)), rng.uniform(-np.pi, np.pi, B), rng.uniform(0.1, 1.0, B)])


def time_launch(make, steps, reps):
    ctl = make()                                                        # waypoints are prepared on the host, once
    names = [n for n in STATE if torch.is_tensor(getattr(ctl, n, None))]
    start = {n: getattr(ctl, n).clone() for n in names}
    ms = []
    for rep in range(reps + 1):
        for n in names:
            getattr(ctl, n).copy_(start[n])
        ctl.steps_done = 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctl.control_step(steps)
        e1.record()
        torch.cuda.synchronize()
        if rep > 0:                                                     # the first launch is the warm-up
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms), int((ctl.ret != 0).sum())


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    obs, wps = scene()
    for B in (4096, 65536):
        X0 = starts(B)
        for model in SPECS:
            def yardstick():
                c = sca.BatchedTrackingController(X0, dict(SPECS[model], num_constraints=1), enable_rotation=False, obs=obs)
                c.set_waypoints(wps)
                return c

            def od():
                c = sca.BatchedTrackingController(X0, dict(SPECS[model]), controller_type={"pos": "optimal_decay_cbf_qp"},
                                                  enable_rotation=False, obs=obs)
                c.set_waypoints(wps)
                return c

            os.environ["SC_TRACK_LANE_PER_AGENT"] = "1"
            try:
                y = time_launch(yardstick, steps, reps)
            finally:
                os.environ.pop("SC_TRACK_LANE_PER_AGENT", None)
            o = time_launch(od, steps, reps)
            print(f"B={B:6d} {model:26s} cbf_qp/1 {y[0]:8.3f} ms ({y[1]:.3f} .. {y[2]:.3f}) per {steps} steps, {y[3]} agents ended")
            print(f"B={B:6d} {model:26s} od       {o[0]:8.3f} ms ({o[1]:.3f} .. {o[2]:.3f})  x{o[0] / y[0]:.3f} of cbf_qp/1, {o[3]} agents ended",
                  flush=True)


if __name__ == "__main__":
    main()
