"""GPU parity tests for the argument order of the CBF-QP kernels (csrc/cbf_qp_kernel.hpp): inputs first and preloaded into SGPRs,
controller constants computed on the host and passed by value, every input load issued before the first wait, h stored ahead of the
solve.  None of that may change a result, so every case is held to the C oracle by test_cbfqp_gpu.compare itself -- its tolerances,
its status rule -- with only the launch swapped: each problem is solved twice, with and without an h buffer, and the two launches
must agree bit for bit on u and status.

Shapes: the smallest that reach every edge of the group mapping (G lanes per agent, 64 / G agents per wave): B = 1, 7, 8, 9 (one
wave, partly and exactly filled at G = 8, one agent into the next wave) and 65; K = 1, 3, 8 (G = 8), 16 (G = 16), 20 (G = 32).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_cbfqp_gpu as T  # noqa: E402  (compare, margins, tolerances: the yardstick, used as it is)
from oracle import robots as R  # noqa: E402
import safe_control_amd as sca  # noqa: E402
from safe_control_amd import workloads as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [("f32", "f32", 0.995), ("f32", "f64", 1.0), ("f64", "f64", 1.0)]          # io, compute, share within tolerance (test_config2_du_4096x8)


def run_with_and_without_h(spec, X, u_ref, obs, io="f32", comp="f64", n_obs=None):
    """test_cbfqp_gpu.run_gpu plus a second launch with h_out absent, which must return the same u and status."""
    ctl = sca.BatchedCBFQP(dict(spec), dt=0.05, io_dtype=io, compute_dtype=comp)
    td = ctl.torch_dtype
    tX = torch.tensor(X, dtype=td, device=T.DEV)
    tu = torch.tensor(u_ref, dtype=td, device=T.DEV)
    to = torch.tensor(obs, dtype=td, device=T.DEV)
    tn = None if n_obs is None else torch.tensor(n_obs, dtype=torch.int32, device=T.DEV)
    u, st, h = ctl.solve(tX, tu, to, tn)
    u2, st2, h2 = ctl.solve(tX, tu, to, tn, want_h=False)
    torch.cuda.synchronize()
    assert h2 is None
    assert torch.equal(st, st2) and torch.equal(u.nan_to_num(nan=7.0), u2.nan_to_num(nan=7.0)), "the launch without h_out differs"
    seen = (tX.double().cpu().numpy(), tu.double().cpu().numpy(), to.double().cpu().numpy())
    return u.double().cpu().numpy(), st.cpu().numpy(), h.double().cpu().numpy(), seen


def n_obs_cases(B, K, rng):
    return [None, np.zeros(B, np.int32), np.full(B, K, np.int32), rng.integers(0, K + 1, B).astype(np.int32)]


def group_edge_case(B, K):
    """Seeded inputs for one (B, K): per-agent obstacles, a shared table and the four n_obs settings.  compare() measures u over
    the problems that are optimal, so it needs one in every batch: the seed is advanced until the ORACLE finds one in each of
    the eight (with B = 1 and 20 obstacles most draws are infeasible)."""
    ospec, cp = T.oracle_spec(R.MODEL_DU, T.du_spec()), T.ocbf.default_cbf_param(R.MODEL_DU)
    for seed in range(1000 * K + B, 1000 * K + B + 400):
        rng = np.random.default_rng(seed)
        X, goal, u_ref, obs = W.du_cbfqp_batch(B, K, seed=seed)
        table = np.zeros((K, 7))
        table[:, 0:2] = rng.uniform(0, 14, (K, 2)); table[:, 2] = rng.uniform(0.2, 0.6, K)
        cases = []
        for o in (obs, table):                               # obs_shared 0 and 1
            for n_obs in n_obs_cases(B, K, rng):
                o2 = o
                if n_obs is not None and o.ndim == 3:
                    o2 = o.copy()
                    for i in range(B):
                        o2[i, n_obs[i]:] = 1e30              # what lies beyond n_obs must be ignored
                cases.append((o2, n_obs))
        if all((T.c_oracle.cbfqp_batch(R.MODEL_DU, X, u_ref, o, ospec, cp, 0.05, "cbf", n)[1] == 0).any() for o, n in cases):
            return X, u_ref, cases
    raise AssertionError("no seed with an optimal problem in every batch")


@pytest.mark.parametrize("K", [1, 3, 8, 16, 20])
@pytest.mark.parametrize("B", [1, 7, 8, 9, 65])
def test_every_group_edge(B, K, monkeypatch):
    """n_obs absent / all 0 / all K / mixed, per-agent obstacles and a shared table, h_out present and absent, the three dtype pairs."""
    monkeypatch.setattr(T, "run_gpu", run_with_and_without_h)
    X, u_ref, cases = group_edge_case(B, K)
    for o, n_obs in cases:
        for io, comp, frac in DTYPES:
            T.compare(R.MODEL_DU, T.du_spec(), X, u_ref, o, io, comp, n_obs=n_obs, frac_ok=frac)


def test_hard_mode_reads_the_host_reciprocals(monkeypatch):
    """The hard CBF mode is the one that uses inv_dt and inv_dt2, now divided on the host."""
    monkeypatch.setattr(T, "run_gpu", run_with_and_without_h)
    X, goal, u_ref, obs = W.du_cbfqp_batch(65, 8, seed=21)
    spec = T.du_spec(); spec["cbf_mode"] = "hard"
    T.compare(R.MODEL_DU, spec, X, u_ref, obs, "f64", "f64", cbf_mode="hard")


CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import safe_control_amd as sca
d = np.load(sys.argv[2])
ctl = sca.BatchedCBFQP({"model": "DynamicUnicycle2D", "a_max": 1.0, "w_max": 0.5, "radius": 0.25}, dt=0.05, io_dtype=sys.argv[4], compute_dtype=sys.argv[5])
t = lambda a: torch.tensor(a, dtype=ctl.torch_dtype, device="cuda:0")
tX, tu, to = t(d["X"]), t(d["u"]), t(d["o"])
tn = torch.tensor(d["n"], device="cuda:0")
u, st, h = ctl.solve(tX, tu, to, tn)
u2, st2, _ = ctl.solve(tX, tu, to, tn, want_h=False)
torch.cuda.synchronize()
assert torch.equal(st, st2) and torch.equal(u.nan_to_num(nan=7.0), u2.nan_to_num(nan=7.0))
np.savez(sys.argv[3], u=u.double().cpu().numpy(), st=st.cpu().numpy(), h=h.double().cpu().numpy(),
         X=tX.double().cpu().numpy(), ur=tu.double().cpu().numpy(), o=to.double().cpu().numpy())
"""


@pytest.mark.parametrize("env,K,io,comp", [({"SC_COOP_MAX_AGENTS": "0"}, 8, "f32", "f64"), ({"SC_FORCE_LDS_KERNEL": "1"}, 12, "f64", "f64")],
                         ids=["lane_per_qp_kernel", "lds_kernel"])
def test_the_other_two_kernels(env, K, io, comp, tmp_path, monkeypatch):
    """cbfqp_reg_kernel and the LDS-staged cbfqp_kernel got the same argument order and load order.  Both switches are read once
    per process, so the launch runs in a fresh child; B = 300 is two blocks of the first kernel and five of the second, the last one
    partly filled; ragged obstacle counts take the n_obs load that used to wait on its own."""
    B = 300
    X, goal, u_ref, obs = W.du_cbfqp_batch(B, K, seed=300 + K)
    n_obs = np.random.default_rng(K).integers(0, K + 1, B).astype(np.int32)

    def run_in_child(spec, X, u_ref, obs, io="f32", comp="f64", n_obs=None):
        inp, outp = tmp_path / "in.npz", tmp_path / "out.npz"
        np.savez(inp, X=X, u=u_ref, o=obs, n=n_obs)
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(inp), str(outp), io, comp], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        d = np.load(outp)
        return d["u"], d["st"], d["h"], (d["X"], d["ur"], d["o"])

    monkeypatch.setattr(T, "run_gpu", run_in_child)
    T.compare(R.MODEL_DU, T.du_spec(), X, u_ref, obs, io, comp, n_obs=n_obs)
