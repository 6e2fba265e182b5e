#!/usr/bin/env python3
"""ms per 200 control steps of the fused Quad2D closed loop (sc_tracking_quad2d_rollout_batch, csrc/tracking_quad_qp.hip) beside the
only way to fly Quad2D under 'cbf_qp' without it: three launches per control step, with no host copy between them,

    sc_quadtrack_select_batch -> sc_cbfqp_solve_batch -> sc_quadtrack_apply_batch                      (the yardstick)

on the scene of tests/test_tracking_quad2d_qp_gpu.py (tests/_quad2d_qp_tracking_oracle.py: scene; four circles, two-waypoint climbs)
at B = 4096 and 65536 agents.  The fused loop runs the 200 steps in ONE launch: 'cbf_qp' with K = 3 (as the yardstick) and K = 10 (the
reference's default), and 'optimal_decay_cbf_qp'.  HIP events around the 200 steps, one warm-up of every variant, then the variants
take turns `reps` times; median (min .. max) per variant.  The yardstick's apply kernel takes no solver status: an agent whose QP is
infeasible gets a NaN input and is not frozen, which changes what it computes, not how much.

Usage: python tools/time_quad2d_loop.py [steps] [reps]"""
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _quad2d_qp_tracking_oracle as Q  # noqa: E402
import safe_control_amd as sca  # noqa: E402
from safe_control_amd import _lib  # noqa: E402

DEV = "cuda:0"
STATE = ("X", "state_machine", "current_goal_index", "goal", "ret", "ret_step", "u_pos", "omega", "min_h")


class Resettable:
    def __init__(self, ctl):
        self.ctl = ctl
        self.names = [n for n in STATE if torch.is_tensor(getattr(ctl, n, None))]
        self.start = {n: getattr(ctl, n).clone() for n in self.names}

    def reset(self):
        for n in self.names:
            getattr(self.ctl, n).copy_(self.start[n])
        self.ctl.steps_done = 0


class Fused(Resettable):
    def __init__(self, X0, wps, obs, controller, K):
        ctl = sca.BatchedTrackingController(X0, dict(Q.SPEC, num_constraints=K), controller_type={"pos": controller}, obs=obs)
        ctl.set_waypoints(list(wps))
        super().__init__(ctl)

    def run(self, steps):
        self.ctl.control_step(steps)


class ThreeLaunches(Resettable):
    """select -> CBF-QP -> apply per step on device tensors, as a user of the parent commit would write it."""

    def __init__(self, X0, wps, obs, K):
        ctl = sca.BatchedTrackingController(X0, dict(Q.SPEC, num_constraints=K), controller_type={"pos": "cbf_qp"}, obs=obs)
        ctl.set_waypoints(list(wps))
        super().__init__(ctl)
        rs, n = ctl.robot_spec, ctl.B
        self.lib, self.K, self.M = _lib.load(), K, int(ctl.obs.shape[0])
        p = self.p = _lib.QuadTrackParams()
        p.model, p.io_dtype, p.max_waypoints, p.waypoints_shared = 0, _lib.DTYPE_F64, int(ctl.waypoints.shape[1]), 0
        p.enable_rotation, p.num_constraints = 1, K
        p.dt, p.reached_threshold, p.rotation_threshold, p.robot_radius = ctl.dt, ctl.reached_threshold, ctl.rotation_threshold, float(rs["radius"])
        p.mass, p.inertia, p.f_min, p.f_max = float(rs["mass"]), float(rs["inertia"]), float(rs["f_min"]), float(rs["f_max"])
        t64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=DEV)
        self.wps3, self.goal4 = t64(n, ctl.waypoints.shape[1], 3), t64(n, 4)
        self.wps3[:, :, :2] = ctl.waypoints
        self.obs_sel, self.goal2, self.u_ref, self.track = t64(n, K, 7), t64(n, 2), t64(n, 2), torch.zeros(n, dtype=torch.int32, device=DEV)
        self.solver = sca.BatchedCBFQP(dict(rs), dt=ctl.dt, io_dtype="f64", compute_dtype="f64", cbf_param=dict(ctl.cbf_param))
        self.out = (t64(n, 2), torch.zeros(n, dtype=torch.int32, device=DEV), None)

    def reset(self):
        super().reset()
        self.goal4[:, :2], self.goal4[:, 3] = self.ctl.goal[:, :2], self.ctl.goal[:, 2]

    def run(self, steps):
        c, p, lib = self.ctl, self.p, self.lib
        stream = torch.cuda.current_stream(c.device).cuda_stream
        for k in range(steps):
            rc = lib.sc_quadtrack_select_batch(C.byref(p), c.B, self.M, c.X.data_ptr(), self.wps3.data_ptr(), c.n_wp.data_ptr(),
                                               c.current_goal_index.data_ptr(), c.state_machine.data_ptr(), self.goal4.data_ptr(),
                                               c.obs.data_ptr(), c.ret.data_ptr(), self.obs_sel.data_ptr(), self.goal2.data_ptr(),
                                               self.u_ref.data_ptr(), self.track.data_ptr(), stream)
            _lib.check(rc, "sc_quadtrack_select_batch")
            u, _, _ = self.solver.solve(c.X, self.u_ref, self.obs_sel, want_h=False, out=self.out)
            rc = lib.sc_quadtrack_apply_batch(C.byref(p), c.B, self.M, k, c.X.data_ptr(), c.state_machine.data_ptr(), self.goal4.data_ptr(),
                                              c.obs.data_ptr(), u.data_ptr(), c.u_pos.data_ptr(), c.ret.data_ptr(), c.ret_step.data_ptr(), stream)
            _lib.check(rc, "sc_quadtrack_apply_batch")


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    for B in (4096, 65536):
        X0, wps, obs = Q.scene(B, seed=0)
        variants = {"three launches K=3": ThreeLaunches(X0, wps, obs, 3), "fused cbf_qp K=3": Fused(X0, wps, obs, "cbf_qp", 3),
                    "fused cbf_qp K=10": Fused(X0, wps, obs, "cbf_qp", 10), "fused optimal decay": Fused(X0, wps, obs, "optimal_decay_cbf_qp", 10)}
        ms = {name: [] for name in variants}
        for rep in range(reps + 1):                                      # the first round is the warm-up
            for name, v in variants.items():
                v.reset()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                v.run(steps)
                e1.record()
                torch.cuda.synchronize()
                if rep > 0:
                    ms[name].append(e0.elapsed_time(e1))
        base = statistics.median(ms["three launches K=3"])
        for name, v in variants.items():
            m = statistics.median(ms[name])
            print(f"B={B:6d} {name:20s} {m:9.3f} ms ({min(ms[name]):.3f} .. {max(ms[name]):.3f}) per {steps} steps, x{m / base:.3f} of the "
                  f"three launches, {int((v.ctl.ret != 0).sum())} agents ended", flush=True)


if __name__ == "__main__":
    main()
