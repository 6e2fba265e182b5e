"""Per-launch time of several builds of the headline CBF-QP launch (4096 agents x 8 rows, a 200-node hipGraph), by the protocol of the
attribution ladder of DESIGN.md 1b: every library is loaded into ONE process, each captures its own graph, the graphs are replayed
round-robin 15 times, and the median per launch is printed with the spread.  Written for the empty-body builds that time the
wave-launch ramp (`-DSC_EXP_EMPTY -DSC_EXP_GRID=n`, with `-mllvm -amdgpu-kernarg-preload-count=0|4|16`), it times any variant.
SC_CBFQP_GENERIC=1 in the environment keeps every library on the generic kernel.
    python3 tools/exp_launch_ramp.py exp_libs/lib_a.so exp_libs/lib_b.so ..."""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import safe_control_amd as sca
from safe_control_amd import _lib as _L
from safe_control_amd import workloads as W

dev, B, K, N, REPLAYS = "cuda:0", 4096, 8, 200, 15
X, goal, ur, obs = W.du_cbfqp_batch(B, K, seed=0)
t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
a, b, c = t(X), t(ur), t(obs)
out = (torch.empty((B, 2), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev),
       torch.empty((B, K), dtype=torch.float32, device=dev))
s = torch.cuda.Stream()
graphs = []
for path in sys.argv[1:]:
    lib = C.CDLL(os.path.abspath(path))
    lib.sc_cbfqp_solve_batch.restype, lib.sc_cbfqp_solve_batch.argtypes = _L.SYMBOLS["sc_cbfqp_solve_batch"]
    ctl = sca.BatchedCBFQP({"model": "DynamicUnicycle2D", "a_max": 1.0, "w_max": 0.5, "radius": 0.25}, io_dtype="f32", compute_dtype="f64")
    ctl._lib = lib
    with torch.cuda.stream(s):
        for _ in range(3):
            ctl.solve(a, b, c, None, out=out)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(N):
                ctl.solve(a, b, c, None, out=out)
        g.replay()
    torch.cuda.synchronize()
    graphs.append((os.path.basename(path), g, []))
for _ in range(REPLAYS):
    for name, g, times in graphs:
        with torch.cuda.stream(s):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s); g.replay(); e1.record(s)
        torch.cuda.synchronize()
        times.append(1e3 * e0.elapsed_time(e1) / N)
for name, g, times in graphs:
    print(f"{name}: median {statistics.median(times):.3f} us per launch, min {min(times):.3f}, max {max(times):.3f} ({REPLAYS} replays)")
