#!/usr/bin/env python3
"""ms per control step of the fused Gatekeeper / MPS closed loop on the drift-car scenario (sc_drift_shield_rollout_batch), at
B = 4096 and 65536 cars: the high-friction scene of examples/drift_car/test_drift.py with perturbed starts (HIP events around
n_ctrl-step launches, the first launch excluded), the cost of one call when the caller
supplies the nominal trajectory (no planner chain on the device), and the float64 oracle's car-steps per second on one host core.
Usage: python tools/time_drift_shield.py [steps]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from safe_control_amd.shielding.drift import BatchedDriftShield  # noqa: E402
import _drift_shield_oracle as O  # noqa: E402

MOBS = np.array([[50.0, 0.0, 2.0, 0.0, 4.5, 2.0, 1.0], [35.0, 4.0, 0.75, 0.0, 4.5, 2.0, 1.0]])   # create_high_friction_test


def starts(B, seed=1):
    rng = np.random.default_rng(seed)
    X = np.zeros((B, 8))
    X[:, 0] = 1.0 + rng.uniform(0.0, 20.0, B)
    X[:, 1] = 4.0 + rng.uniform(-0.5, 0.5, B)
    X[:, 5] = 10.0 + rng.uniform(-2.0, 2.0, B)
    return X


def time_gpu(algo, backup, B, steps, reps=3):
    sh = BatchedDriftShield(algo, backup)
    X0 = starts(B)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    best = None
    for rep in range(reps + 1):
        X, fr, mob, st = t(X0), t(np.ones(B)), t(np.repeat(MOBS[None], B, axis=0)), sh.new_state(B, "cuda")
        ret = torch.zeros(B, dtype=torch.int32, device="cuda")
        rs = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sh.rollout(X, fr, mob, st, ret, rs, steps)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / steps
        if rep > 0:
            best = ms if best is None else min(best, ms)
    return best, int((ret != 0).sum())


def time_step_external(algo, backup, B, reps=5, distinct=64):
    """ms per solve_control_problem launch (sc_drift_shield_step_batch, fresh shields: every call is an event) when the caller
    supplies the nominal trajectory, so that no planner chain runs on the device: what the shield itself costs.  The plans are
    the oracle's lane keeper from `distinct` start states, tiled over the batch."""
    sh = BatchedDriftShield(algo, backup)
    X0 = starts(distinct)
    plans = [O.nominal_rollout(x, sh.n_nominal, O.default_track(), 1.0, O.default_spec(), sh.dt) for x in X0]
    tile = lambda a: np.tile(a, (B // distinct,) + (1,) * (a.ndim - 1))
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    X, nx, nu = t(tile(X0)), t(tile(np.array([p[0] for p in plans]))), t(tile(np.array([p[1] for p in plans])))
    fr, mob = t(np.ones(B)), t(np.repeat(MOBS[None], B, axis=0))
    best = None
    for rep in range(reps + 1):
        st = sh.new_state(B, "cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sh.step(X, fr, st, nx, nu, moving_obs=mob)
        e1.record()
        torch.cuda.synchronize()
        if rep > 0:
            best = e0.elapsed_time(e1) if best is None else min(best, e0.elapsed_time(e1))
    return best


def time_oracle(algo, backup, n=4, steps=10):
    X0 = starts(n)
    c = O.stop_ctrl(O.default_spec()) if backup == "stop" else O.lane_change_ctrl(O.default_spec(), -4.0)
    t0 = time.perf_counter()
    for i in range(n):
        O.replay(algo, c, X0[i], MOBS, 1.0, steps - 1)
    return n * steps / (time.perf_counter() - t0)


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    for algo, aid in (("gatekeeper", O.GATEKEEPER), ("mps", O.MPS)):
        for backup in ("lane_change", "stop"):
            for B in (4096, 65536):
                ms, done = time_gpu(algo, backup, B, steps)
                print(f"{algo:10s} {backup:11s} B={B:6d}  {ms:8.3f} ms per control step ({B / ms / 1e3:7.2f} M car-steps/s; {done} cars ended in {steps} steps)",
                      flush=True)
            print(f"{algo:10s} {backup:11s} B=  4096  {time_step_external(algo, backup, 4096):8.3f} ms per call with a caller-supplied nominal trajectory (no planner on the device)",
                  flush=True)
            print(f"{algo:10s} {backup:11s} oracle  {time_oracle(aid, backup):8.1f} car-steps/s on one host core", flush=True)


if __name__ == "__main__":
    main()
