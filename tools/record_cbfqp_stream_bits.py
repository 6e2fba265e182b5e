"""Records tests/golden/cbfqp_stream_bits.npz: u, status and h of the cooperative CBF-QP kernel on every case of
workloads.cbfqp_stream_cases(), as raw bit patterns (NaNs of the infeasible agents included), for tests/test_cbfqp_stream_gpu.py.

The committed fixture was recorded on one MI355X at commit 0d06ede ("Preload CBF-QP kernel arguments and fetch the rest under the
loads"), i.e. from the build BEFORE the instruction stream of the cooperative kernel was shortened; the test holds every later
build to it bit for bit.  Run it again only from a build whose results are the reference on purpose.

    python3 tools/record_cbfqp_stream_bits.py [OUT.npz]      (SAFE_CONTROL_AMD_LIB selects the library)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import safe_control_amd as sca
from safe_control_amd import workloads as W

SPEC = {"model": "DynamicUnicycle2D", "a_max": 1.0, "w_max": 0.5, "radius": 0.25}
BITS = {np.dtype("float32"): np.uint32, np.dtype("float64"): np.uint64}


def solve_bits(io, comp, mode, X, u_ref, obs, n_obs, dev="cuda:0"):
    """One launch; the outputs as unsigned integers of the storage width, so that comparing them compares every bit."""
    ctl = sca.BatchedCBFQP(dict(SPEC, cbf_mode=mode), dt=0.05, io_dtype=io, compute_dtype=comp)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=ctl.torch_dtype, device=dev)
    tn = None if n_obs is None else torch.tensor(n_obs, dtype=torch.int32, device=dev)
    u, st, h = ctl.solve(t(X), t(u_ref), t(obs), tn)
    torch.cuda.synchronize()
    u, h = u.cpu().numpy(), h.cpu().numpy()
    return u.view(BITS[u.dtype]), st.cpu().numpy().astype(np.int32), h.view(BITS[h.dtype])


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "cbfqp_stream_bits.npz")
    rec = {}
    for name, io, comp, mode, X, u_ref, obs, n_obs in W.cbfqp_stream_cases():
        u, st, h = solve_bits(io, comp, mode, X, u_ref, obs, n_obs)
        rec[name + ".u"], rec[name + ".status"], rec[name + ".h"] = u, st, h
        print(f"{name}: {int((st == 0).sum())} optimal, {int((st == 1).sum())} infeasible, {int((st == 3).sum())} bad obstacle")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
