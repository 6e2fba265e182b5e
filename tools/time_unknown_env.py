#!/usr/bin/env python3
"""ms per launch of the sensing rollout (sc_tracking_sense_rollout_batch, csrc/tracking_sense.hip) beside the plain lane-per-agent
rollout it grew from (sc_tracking_rollout_batch with SC_TRACK_LANE_PER_AGENT=1), on the 14-circle scene of
tests/golden/closed_loop.npz: B = 4096 and 65536 agents x 200 control steps in one launch, HIP events around the launch, one
warm-up launch, median (and min .. max) of the repeated runs.

  plain      the parent's lane-per-agent rollout                                   (1)
  sense/0    the sensing rollout without unknown rows: same arithmetic as (1),     (2)
             so (2) / (1) is what the added per-agent state and the empty scans cost
  sense/16, sense/64   DoubleIntegrator2D turning under 'velocity_tracking_yaw'     (3)
             with 0, 16 and 64 unknown circles: the difference to its own Mu = 0
             row is the detection scan and the two collision scans over the unknown table

  mpc        the select / solve / apply loops under 'mpc_cbf' with the tuning of            (4)
             examples/test_unknown_env.py (:197-206), B = 4096, ms per CONTROL STEP:
             BatchedTrackingController (sc_tracking_select_batch / _apply_batch around
             the MPC launch) beside BatchedSensingMPCTrackingController
             (sc_tracking_sense_select_batch / _apply_batch, csrc/tracking_sense_split.hip)
             with 0 and 16 unknown circles; the Mu = 0 ratio is what the sensing pair costs

Usage: python tools/time_unknown_env.py [steps] [reps]          legs (1) - (3)
       python tools/time_unknown_env.py mpc [steps] [reps]      leg (4) alone (20 steps, 3 repetitions by default)"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import safe_control_amd as sca  # noqa: E402

SPECS = {"DynamicUnicycle2D": {"model": "DynamicUnicycle2D", "a_max": 1.0, "w_max": 0.5, "radius": 0.25},
         "DoubleIntegrator2D": {"model": "DoubleIntegrator2D", "v_max": 1.0, "a_max": 1.0, "radius": 0.25}}


def scene():
    g = np.load(os.path.join(ROOT, "tests", "golden", "closed_loop.npz"))
    return g["du14/obs"], g["du14/waypoints"][:, :2]


def starts(model, B, seed=1):
    rng = np.random.default_rng(seed)
    pos = 2.0 + rng.uniform(-0.4, 0.4, (B, 2))
    yaw = rng.uniform(-np.pi, np.pi, B)
    if model == "DynamicUnicycle2D":
        return np.column_stack([pos, yaw, rng.uniform(0, 1, B)])
    return np.column_stack([pos, rng.uniform(-0.3, 0.3, (B, 2)), yaw])


def unknown_rows(Mu, seed=2):
    """Mu small circles scattered over the scene (no two within the memory's merge tolerance: they are a grid's cells)."""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(14 * 14)[:Mu]
    return np.column_stack([cells % 14 + rng.uniform(0.2, 0.8, Mu), cells // 14 + rng.uniform(0.2, 0.8, Mu), rng.uniform(0.1, 0.2, Mu)])


STATE = ("X", "state_machine", "current_goal_index", "goal", "ret", "ret_step", "u_pos", "yaw", "u_att", "seen",
         "u_prev", "mpc_status", "mpc_iters")
# examples/test_unknown_env.py:197-206 (apply_algo_tuning) under --algo mpc_cbf
MPC_TUNING = {"DynamicUnicycle2D": {"mpc_horizon": 7, "mpc_cbf_alpha1": 0.26, "mpc_cbf_alpha2": 0.26},
              "DoubleIntegrator2D": {"mpc_horizon": 9, "mpc_cbf_alpha1": 0.32, "mpc_cbf_alpha2": 0.32}}


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


def mpc_leg(steps, reps, B=4096):
    """Leg (4): ms per control step of the MPC loops; the plain class is the yardstick (no unknown rows, the same rotation flag)."""
    obs, wps = scene()
    mpc = {"pos": "mpc_cbf"}
    for model, rot in (("DynamicUnicycle2D", True), ("DoubleIntegrator2D", False)):
        X0 = starts(model, B)
        spec = dict(SPECS[model], **MPC_TUNING[model])

        def plain():
            c = sca.BatchedTrackingController(X0, dict(spec), controller_type=mpc, enable_rotation=rot, obs=obs)
            c.set_waypoints(wps)
            return c

        p = time_launch(plain, steps, reps)
        tag = f"{model}{'' if rot else ' (enable_rotation=False)'}"
        print(f"B={B:6d} {tag:42s} mpc plain     {p[0] / steps:8.3f} ms per control step ({p[1] / steps:.3f} .. {p[2] / steps:.3f}), "
              f"{p[3]} agents ended in {steps} steps")
        for Mu in (0, 16):
            def sense():
                c = sca.BatchedSensingMPCTrackingController(X0, dict(spec), controller_type=mpc, enable_rotation=rot, obs=obs,
                                                            unknown_obs=unknown_rows(Mu))
                c.set_waypoints(wps)
                return c
            s = time_launch(sense, steps, reps)
            print(f"B={B:6d} {tag:42s} mpc sense/{Mu:<2d}  {s[0] / steps:8.3f} ms per control step ({s[1] / steps:.3f} .. {s[2] / steps:.3f})  "
                  f"x{s[0] / p[0]:.3f} of plain, {s[3]} agents ended")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "mpc":
        return mpc_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 20, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    obs, wps = scene()
    for B in (4096, 65536):
        for model, rot in (("DynamicUnicycle2D", True), ("DoubleIntegrator2D", False)):
            X0 = starts(model, B)

            def plain():
                c = sca.BatchedTrackingController(X0, dict(SPECS[model]), enable_rotation=rot, obs=obs)
                c.set_waypoints(wps)
                return c

            def sense0():
                c = sca.BatchedSensingTrackingController(X0, dict(SPECS[model]), enable_rotation=rot, obs=obs)
                c.set_waypoints(wps)
                return c

            os.environ["SC_TRACK_LANE_PER_AGENT"] = "1"
            try:
                p = time_launch(plain, steps, reps)
            finally:
                os.environ.pop("SC_TRACK_LANE_PER_AGENT", None)
            s = time_launch(sense0, steps, reps)
            tag = f"{model}{'' if rot else ' (enable_rotation=False)'}"
            print(f"B={B:6d} {tag:42s} plain    {p[0]:8.3f} ms ({p[1]:.3f} .. {p[2]:.3f}) per {steps} steps, {p[3]} agents ended")
            print(f"B={B:6d} {tag:42s} sense/0  {s[0]:8.3f} ms ({s[1]:.3f} .. {s[2]:.3f})  x{s[0] / p[0]:.3f} of plain")
        X0 = starts("DoubleIntegrator2D", B)
        base = None
        for Mu in (0, 16, 64):
            def sense():
                c = sca.BatchedSensingTrackingController(X0, dict(SPECS["DoubleIntegrator2D"]), obs=obs, unknown_obs=unknown_rows(Mu))
                c.set_waypoints(wps)
                return c
            s = time_launch(sense, steps, reps)
            base = s[0] if base is None else base
            print(f"B={B:6d} {'DoubleIntegrator2D, velocity_tracking_yaw':42s} sense/{Mu:<2d} {s[0]:8.3f} ms ({s[1]:.3f} .. {s[2]:.3f})  "
                  f"+{s[0] - base:.3f} ms over Mu = 0, {s[3]} agents ended")


if __name__ == "__main__":
    main()
