"""The benchmark batch runs the straight path of cbfqp_coop8_du_kernel (csrc/cbf_qp_kernel.hpp).

CPU only.  The specialised cooperative CBF-QP kernel treats every lane as ordinary and sends a wave that holds a lane which is
not to the generic K = 8 sequence, through one of two wave-uniform exits:

  * early: some row's flag is not 0 (`noncircle`; a flag that is neither 0 nor 1, `bad`, is one of these), or not |theta| < 1e5;
  * late: some row without nn > 0 (`degenerate`), or, in a wave that enters the solve, a unit normal with a component that is
    exactly 0 (`flat`) or two rows of one agent with |n_i x n_j| <= eps_par (`par`).

With tools/count_coop8_branches.conditions on the batch bench.py measures -- workloads.du_cbfqp_batch(4096, 8, seed=0), rounded
to f32 storage as the benchmark stores it -- no wave meets any of them, so all 512 waves of the headline launch take the fast
path from the entry to its stores.  The late conditions are counted in every wave, entering the solve or not, which is the
stronger statement.
"""
import os
import sys

import numpy as np
import pytest

from oracle import robots as R
from safe_control_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import count_coop8_branches as CB  # noqa: E402

AGENTS, ROWS, TH_MAX = 4096, 8, 1.0e5


@pytest.fixture(scope="module")
def bench_conditions():
    X, _, u_ref, obs = W.du_cbfqp_batch(AGENTS, ROWS, seed=0)
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32).astype(np.float64)
    X, u_ref, obs = f32(X), f32(u_ref), f32(obs)
    spec = R.default_spec(R.MODEL_DU)
    spec.update(a_max=1.0, w_max=0.5, radius=0.25)
    c = CB.conditions(X, u_ref, obs, spec)
    c["theta"] = ~(np.abs(X[:, 2]) < TH_MAX)
    return c


def waves(per_agent):
    """Agents -> waves of 8 agents: does any agent of the wave meet the condition?"""
    assert per_agent.shape == (AGENTS,)
    return per_agent.reshape(-1, 8).any(axis=1)


def test_the_batch_is_the_headline_launch(bench_conditions):
    enters = waves(bench_conditions["viol"].any(axis=1))
    print(f"{len(enters)} waves, {int(enters.sum())} enter the solve")
    assert len(enters) == 512 and enters.sum() > 400, "the slowest wave of the launch is one that enters the solve"


@pytest.mark.parametrize("key", ("noncircle", "theta", "degenerate", "flat", "par", "bad"))
def test_no_wave_meets_an_exit_condition(bench_conditions, key):
    m = bench_conditions[key]
    per_agent = m if m.ndim == 1 else m.reshape(AGENTS, -1).any(axis=1)
    n = int(waves(per_agent).sum())
    print(f"{key}: {n} waves")
    assert n == 0


def test_distance_to_the_thresholds(bench_conditions):
    """Not within rounding of a threshold: the oracle's rows differ from the kernel's in the last bits only."""
    print(f"smallest |component| of a unit normal {bench_conditions['min_comp']:.3e}, smallest |n_i x n_j| {bench_conditions['min_cross']:.3e}")
    assert bench_conditions["min_comp"] > 1e-9 and bench_conditions["min_cross"] > 1e3 * CB.EPS_PAR
