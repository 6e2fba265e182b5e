#!/usr/bin/env python3
"""ms per control step of the fused Gatekeeper / MPS closed loop (sc_shield_rollout_batch) on the evade scenario, at
B = 4096 and 65536 agents drawn like tests/test_shield_gpu.py (HIP events around n_ctrl-step launches, warm-up launches
excluded), and the float64 oracle's per-agent rate on one host core for context.  Usage: python tools/time_shield.py [steps]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import safe_control_amd as sca  # noqa: E402
import _shield_oracle as SO  # noqa: E402
from test_shield_gpu import draw  # noqa: E402


def time_gpu(algo, B, steps, reps=3):
    sh = sca.BatchedShield(algo)
    X0, bx0 = draw(B, seed=1)
    t = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")
    best = None
    for rep in range(reps + 1):
        X, bx, st = t(X0), t(bx0), sh.new_state(B, "cuda")
        ret = torch.zeros(B, dtype=torch.int32, device="cuda")
        rs = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sh.rollout(X, bx, st, ret, rs, steps)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / steps
        if rep > 0:                                                     # the first launch is the warm-up
            best = ms if best is None else min(best, ms)
    return best, int((ret != 0).sum())


def time_oracle(algo, n=20, steps=10):
    X0, bx0 = draw(n, seed=1)
    t0 = time.perf_counter()
    for i in range(n):
        SO.replay((algo, X0[i], bx0[i], steps - 1, 0.1, 12.0, 10.0, 0.05))
    return n * steps / (time.perf_counter() - t0)


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    for algo, aid in (("gatekeeper", SO.GATEKEEPER), ("mps", SO.MPS)):
        for B in (4096, 65536):
            ms, done = time_gpu(algo, B, steps)
            print(f"{algo:10s} B={B:6d}  {ms:8.3f} ms per control step ({B / ms / 1e3:7.2f} M agent-steps/s; {done} agents ended in {steps} steps)")
        print(f"{algo:10s} oracle  {time_oracle(aid):8.1f} agent-steps/s on one host core")


if __name__ == "__main__":
    main()
