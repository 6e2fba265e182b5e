"""Fleet closed loop at the BASELINE configs[3] size: 16384 KinematicBicycle2D C3BF agents, K_nb = 16 nearest other agents,
M = 16 moving table rows, f32 storage, 200 steps on one GPU (BatchedFleetTrackingController).  Prints ms per step from a host
clock around synchronised steps, the reached / infeasible / collided split and the smallest separation.  The kernels have
stable names (nb_*_kernel, tracking_fleet_kernel, advance_obstacle_table_kernel) for a separate
``rocprofv3 --kernel-trace --stats -- python tools/time_fleet.py`` run.

Usage: python tools/time_fleet.py [n_agents] [steps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import safe_control_amd as sca  # noqa: E402
from safe_control_amd import workloads as W  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    X0, wps, obs = W.kb_c3bf_fleet_scene(n, 16, seed=0)
    ctl = sca.BatchedFleetTrackingController(X0, {"model": "KinematicBicycle2D_C3BF"}, obs=obs, dyn_obs=True, neighbours=16,
                                             io_dtype="f32", device="cuda:0")
    ctl.set_waypoints(list(wps))
    torch.cuda.synchronize()
    per = []
    for _ in range(steps):                                   # one synchronised step at a time: the host clock sees each
        t0 = time.perf_counter()
        ctl.control_step(1)
        torch.cuda.synchronize()
        per.append(time.perf_counter() - t0)
    s = ctl.summary()
    per = np.array(per[5:]) * 1e3
    # the loop as an application runs it: 200 steps back to back, one sync at the end
    ctl2 = sca.BatchedFleetTrackingController(X0, {"model": "KinematicBicycle2D_C3BF"}, obs=obs, dyn_obs=True, neighbours=16,
                                              io_dtype="f32", device="cuda:0")
    ctl2.set_waypoints(list(wps))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctl2.control_step(steps)
    torch.cuda.synchronize()
    stream_ms = (time.perf_counter() - t0) * 1e3 / steps
    assert ctl2.summary() == s, "two runs of the same scene differ"
    print(json.dumps({"agents": n, "steps": steps, "ms_per_step_sync_median": round(float(np.median(per)), 4),
                      "ms_per_step_sync_min": round(float(per.min()), 4), "ms_per_step_streamed": round(stream_ms, 4), "summary": s}))


if __name__ == "__main__":
    main()
